// The finetune objective of compute_losses (base_rendering_model.py:533-664) on the
// device: the colour items (plain / ray_masked_ / ray_miss_ / ray_depth_masked_
// MSE) in one pass with device counts, and the sparse loss (:652-662) per point.
// No host read, no allocation, bitwise repeatable in both directions.
//
// Every sum runs in fp64 (the inputs widened exactly) and is rounded to fp32
// once: these kernels move a few kB to a few MB and are launch-bound, so the
// fp64 rate does not show, and the result is the correctly rounded value of
// the formula instead of one of fp32's summation orders.
#include "pnr_common.h"

namespace pnr {

// ----------------------------------------------------------------- colour losses
// Block b takes the contiguous row range [b per, (b + 1) per) and walks its
// elements (row, channel) in a fixed thread order; waves reduce by shuffles, the
// four waves through LDS in wave order, and one last block adds the kLossBlocks
// partials in block order.  kind 0 = all rays, 1 = ray_mask > 0, 2 = ray_mask == 0,
// 3 = extra_mask > 0.
constexpr int kLossBlocks = 256;

struct ColorLossArgs {
  const float* x;
  int64_t ldx;
  const float* gt;
  int64_t ldgt;
  const int8_t* ray_mask;
  const uint8_t* extra;
  int64_t R;
  int C;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// psum [kLossBlocks][4] doubles, pcnt [kLossBlocks][4] int64 (pcnt[.][0] unused)
__global__ void __launch_bounds__(256) k_color_loss_part(ColorLossArgs a, double* __restrict__ psum,
                                                         long long* __restrict__ pcnt) {
  __shared__ double rs[4][4];
  __shared__ long long rn[4][4];
  const int C = a.C;
  const int64_t per = cdiv(a.R, (int64_t)kLossBlocks);
  const int64_t r0 = blockIdx.x * per;
  const int64_t r1 = r0 + per < a.R ? r0 + per : a.R;
  const int64_t n = r1 > r0 ? (r1 - r0) * C : 0;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long long cnt[4] = {0, 0, 0, 0};
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    const int64_t rr = j / C;
    const int c = (int)(j - rr * C);
    const int64_t r = r0 + rr;
    const double d = (double)a.x[r * a.ldx + c] - (double)a.gt[r * a.ldgt + c];
    const double d2 = d * d;
    const int m = a.ray_mask[r];
    const bool in[4] = {true, m > 0, m == 0, a.extra != nullptr && a.extra[r] != 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (in[k]) {
        s[k] += d2;
        cnt[k] += (c == 0);
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double ws = wave_sum_f64(s[k]);
    const long long wn = wave_sum_i64(cnt[k]);
    if (lane == 0) {
      rs[wid][k] = ws;
      rn[wid][k] = wn;
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    psum[blockIdx.x * 4 + k] = ((rs[0][k] + rs[1][k]) + rs[2][k]) + rs[3][k];
    pcnt[blockIdx.x * 4 + k] = rn[0][k] + rn[1][k] + rn[2][k] + rn[3][k];
  }
}

// out[4]: the four item values; counts[4] = (R, n_hit, n_miss, n_extra)
__global__ void __launch_bounds__(64) k_color_loss_final(const double* __restrict__ psum,
                                                         const long long* __restrict__ pcnt, int C,
                                                         float* __restrict__ out, long long* __restrict__ counts) {
  const int k = threadIdx.x;
  if (k >= 4) return;
  double s = 0.0;
  long long n = 0;
  for (int b = 0; b < kLossBlocks; ++b) {
    s += psum[b * 4 + k];
    n += pcnt[b * 4 + k];
  }
  counts[k] = n;
  // ray_miss_: MSELoss x the number of missed rays (base_rendering_model.py:560) = sum / C
  const double den = (k == 2 ? 1.0 : (double)n) * (double)C;
  out[k] = n > 0 ? (float)(s / den) : 0.f;
}

// d_x[r, c] = 2 (x - g) sum_k g_kind[k] coef_k(r)
__global__ void __launch_bounds__(256) k_color_loss_bwd(ColorLossArgs a, const long long* __restrict__ counts,
                                                        const float* __restrict__ g_kind, float* __restrict__ d_x,
                                                        int64_t ldd) {
  const int C = a.C;
  double coef[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long n = counts[k];
    const double den = (k == 2 ? 1.0 : (double)n) * (double)C;
    coef[k] = n > 0 ? 2.0 * (double)g_kind[k] / den : 0.0;
  }
  const int64_t n = a.R * C;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = j / C;
    const int c = (int)(j - r * C);
    const int m = a.ray_mask[r];
    double cf = coef[0];
    if (m > 0) cf += coef[1];
    if (m == 0) cf += coef[2];
    if (a.extra != nullptr && a.extra[r] != 0) cf += coef[3];
    const double d = (double)a.x[r * a.ldx + c] - (double)a.gt[r * a.ldgt + c];
    d_x[r * ldd + c] = (float)(d * cf);
  }
}

// ------------------------------------------------------------------- sparse loss
// sum(weight |1 - exp(-2 cc)|) / (sum(weight) + 1e-6) per point: W_p = the summed
// weight of the pairs that gather p.  The pair weights are k_march_aux's
// (composite.hip), term by term, from the query's own buffers.  W_p accumulates
// in 64-bit fixed point (kWScale) with integer atomics: integer addition is
// associative, so the sums do not depend on the order the waves arrive in.
constexpr double kWScale = 0x1p38;           // a weight is <= 1: 2^25 pairs fit 63 bits
constexpr int64_t kSparseMaxPairs = 1ll << 25;

struct SparseArgs {
  int64_t R, N, cap;   // rays, points, sample rows of pidx / sample_w
  int SR, K;
  const int32_t* n_filled;
  const int32_t* ray_off;
  const int32_t* ray_vcnt;
  const int32_t* pidx;
  const float* sample_w;
  const float* xyz;
  unsigned long long* wfix;
};

__global__ void __launch_bounds__(256) k_sparse_weights(SparseArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int SR = a.SR, K = a.K;
  for (int64_t r = wave0; r < a.R; r += nwaves) {
    if (a.ray_vcnt[r] <= 0) continue;
    const int n = a.n_filled[r], off = a.ray_off[r];
    for (int s = lane; s < SR && s < n; s += 64) {
      const int64_t i = (int64_t)off + s;
      if (i < 0 || i >= a.cap) continue;
      const float sw[3] = {a.sample_w[i * 3], a.sample_w[i * 3 + 1], a.sample_w[i * 3 + 2]};
      float wl[16];
      int32_t pk[16];
      float sum = 0.f;
      for (int k = 0; k < K; ++k) {
        int32_t p = a.pidx[i * K + k];
        if (p >= a.N) p = -1;
        float v = 0.f;
        if (p >= 0) {
          const float d0 = a.xyz[(int64_t)p * 3] - sw[0], d1 = a.xyz[(int64_t)p * 3 + 1] - sw[1],
                      d2 = a.xyz[(int64_t)p * 3 + 2] - sw[2];
          v = 1.f / fmaxf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2), 1e-6f);
        }
        pk[k] = p;
        wl[k] = v;
        sum += v;
      }
      const float den = fmaxf(sum, 1e-8f);
      for (int k = 0; k < K; ++k) {
        if (pk[k] < 0) continue;
        const float w = wl[k] / den;
        const unsigned long long q = (unsigned long long)__double2ll_rn((double)w * kWScale);
        if (q) atomicAdd(a.wfix + pk[k], q);
      }
    }
  }
}

__device__ __forceinline__ double sparse_cc(const float* conf, int64_t p) {
  return conf ? (double)fminf(fmaxf(conf[p], 1e-4f), 1.f) : 1.0;
}

// pnum [kLossBlocks] doubles: sum_p W_p f(cc_p); pw [kLossBlocks] uint64: sum_p W_p (fixed point)
__global__ void __launch_bounds__(256) k_sparse_part(const unsigned long long* __restrict__ wfix,
                                                     const float* __restrict__ conf, int64_t N,
                                                     double* __restrict__ pnum, unsigned long long* __restrict__ pw) {
  __shared__ double rs[4];
  __shared__ long long rn[4];
  const int64_t per = cdiv(N, (int64_t)kLossBlocks);
  const int64_t b0 = blockIdx.x * per, b1 = b0 + per < N ? b0 + per : N;
  double s = 0.0;
  long long n = 0;
  for (int64_t p = b0 + threadIdx.x; p < b1; p += 256) {
    const unsigned long long q = wfix[p];
    if (q) {
      const double cc = sparse_cc(conf, p);
      s += (double)q * fabs(1.0 - exp(-2.0 * cc));
      n += (long long)q;
    }
  }
  s = wave_sum_f64(s);
  n = wave_sum_i64(n);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rn[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    pnum[blockIdx.x] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
    pw[blockIdx.x] = (unsigned long long)(rn[0] + rn[1] + rn[2] + rn[3]);
  }
}

// out[0] = the loss; state[0] = sum(weight) + 1e-6 (the backward's denominator)
__global__ void __launch_bounds__(64) k_sparse_final(const double* __restrict__ pnum,
                                                     const unsigned long long* __restrict__ pw,
                                                     float* __restrict__ out, double* __restrict__ state) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  unsigned long long n = 0;
  for (int b = 0; b < kLossBlocks; ++b) {
    s += pnum[b];
    n += pw[b];
  }
  const double den = (double)n / kWScale + 1e-6;
  out[0] = (float)(s / kWScale / den);
  state[0] = den;
}

// d conf_p = g W_p f'(cc_p) / (sum W + 1e-6), f' = sign(1 - e) 2 e, e = exp(-2 cc);
// gradiant_clamp passes the gradient straight through (no clamp mask)
__global__ void __launch_bounds__(256) k_sparse_bwd(const unsigned long long* __restrict__ wfix,
                                                    const float* __restrict__ conf, int64_t N,
                                                    const double* __restrict__ state, const float* __restrict__ g,
                                                    float* __restrict__ d_conf) {
  const double scale = (double)g[0] / (state[0] * kWScale);
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long q = wfix[p];
    float d = 0.f;
    if (q) {
      const double e = exp(-2.0 * sparse_cc(conf, p));
      const double sg = e < 1.0 ? 1.0 : (e > 1.0 ? -1.0 : 0.0);
      d = (float)(scale * (double)q * sg * 2.0 * e);
    }
    d_conf[p] = d;
  }
}

}  // namespace pnr

using namespace pnr;

static size_t color_loss_scratch() { return (size_t)kLossBlocks * 4 * (sizeof(double) + sizeof(long long)); }

extern "C" int pnr_color_loss_scratch_bytes(size_t* out) {
  PNR_CHECK_ARG(out, "color_loss_scratch_bytes: null pointer");
  *out = color_loss_scratch();
  return PNR_OK;
}

static int color_loss_args(const char* who, const float* x, int64_t ldx, const float* gt, int64_t ldgt,
                           const int8_t* ray_mask, int64_t R, int32_t C) {
  PNR_CHECK_ARG(R >= 0, "%s: R < 0", who);
  PNR_CHECK_ARG(C >= 1 && C <= 128, "%s: C=%d unsupported (1..128)", who, C);
  PNR_CHECK_ARG((x && gt && ray_mask) || R == 0, "%s: null pointer", who);
  PNR_CHECK_ARG(ldx >= C && ldgt >= C, "%s: row stride below C (ldx %lld, ldgt %lld, C %d)", who, (long long)ldx,
                (long long)ldgt, C);
  return PNR_OK;
}

extern "C" int pnr_color_loss_fwd(const float* x, int64_t ldx, const float* gt, int64_t ldgt, const int8_t* ray_mask,
                                  const uint8_t* extra_mask, int64_t R, int32_t C, float* out, int64_t* counts,
                                  void* scratch, size_t scratch_bytes, void* stream) {
  if (int rc = color_loss_args("color_loss_fwd", x, ldx, gt, ldgt, ray_mask, R, C)) return rc;
  PNR_CHECK_ARG(out && counts && scratch, "color_loss_fwd: null pointer");
  PNR_CHECK_ARG(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)counts & 7) == 0,
                "color_loss_fwd: scratch and counts must be 8-B aligned");
  PNR_CHECK_ARG(scratch_bytes >= color_loss_scratch(), "color_loss_fwd: scratch too small (%zu < %zu)",
                scratch_bytes, color_loss_scratch());
  ColorLossArgs a = {x, ldx, gt, ldgt, ray_mask, extra_mask, R, C};
  double* psum = static_cast<double*>(scratch);
  long long* pcnt = reinterpret_cast<long long*>(psum + kLossBlocks * 4);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_color_loss_part, dim3(kLossBlocks), dim3(256), 0, st, a, psum, pcnt);
  PNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_color_loss_final, dim3(1), dim3(64), 0, st, psum, pcnt, C, out,
                     reinterpret_cast<long long*>(counts));
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_color_loss_bwd(const float* x, int64_t ldx, const float* gt, int64_t ldgt, const int8_t* ray_mask,
                                  const uint8_t* extra_mask, int64_t R, int32_t C, const int64_t* counts,
                                  const float* g_kind, float* d_x, int64_t ldd, void* stream) {
  if (int rc = color_loss_args("color_loss_bwd", x, ldx, gt, ldgt, ray_mask, R, C)) return rc;
  PNR_CHECK_ARG(counts && g_kind && (d_x || R == 0), "color_loss_bwd: null pointer");
  PNR_CHECK_ARG(ldd >= C, "color_loss_bwd: row stride below C (ldd %lld, C %d)", (long long)ldd, C);
  PNR_CHECK_ARG(((uintptr_t)counts & 7) == 0, "color_loss_bwd: counts must be 8-B aligned");
  if (R == 0) return PNR_OK;
  ColorLossArgs a = {x, ldx, gt, ldgt, ray_mask, extra_mask, R, C};
  hipLaunchKernelGGL(k_color_loss_bwd, dim3(grid_for(R * C, 256, 2048)), dim3(256), 0, as_stream(stream), a,
                     reinterpret_cast<const long long*>(counts), g_kind, d_x, ldd);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

static size_t sparse_loss_scratch() { return (size_t)kLossBlocks * (sizeof(double) + sizeof(unsigned long long)); }

extern "C" int pnr_sparse_loss_scratch_bytes(size_t* out) {
  PNR_CHECK_ARG(out, "sparse_loss_scratch_bytes: null pointer");
  *out = sparse_loss_scratch();
  return PNR_OK;
}

extern "C" int pnr_sparse_loss_fwd(const pnr_query_params* q, const pnr_query_bufs* b, int64_t R, const float* xyz,
                                   const float* conf, int64_t N, uint64_t* w_fix, float* out, double* state,
                                   void* scratch, size_t scratch_bytes, void* stream) {
  PNR_CHECK_ARG(q && b && xyz && w_fix && out && state && scratch, "sparse_loss_fwd: null pointer");
  PNR_CHECK_ARG(R >= 0 && N > 0, "sparse_loss_fwd: bad sizes (R %lld, N %lld)", (long long)R, (long long)N);
  PNR_CHECK_ARG(q->SR >= 1 && q->SR <= 128, "sparse_loss_fwd: SR=%d unsupported (1..128)", q->SR);
  PNR_CHECK_ARG(q->K >= 1 && q->K <= 16, "sparse_loss_fwd: K=%d unsupported (1..16)", q->K);
  PNR_CHECK_ARG(R * q->SR * (int64_t)q->K <= kSparseMaxPairs,
                "sparse_loss_fwd: R SR K = %lld pairs exceed the fixed-point range (%lld)",
                (long long)(R * q->SR * (int64_t)q->K), (long long)kSparseMaxPairs);
  PNR_CHECK_ARG(R == 0 || (b->n_filled && b->ray_off && b->ray_vcnt && b->pidx && b->sample_w),
                "sparse_loss_fwd: query buffers missing");
  PNR_CHECK_ARG(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)w_fix & 7) == 0 && ((uintptr_t)state & 7) == 0,
                "sparse_loss_fwd: scratch, w_fix and state must be 8-B aligned");
  PNR_CHECK_ARG(scratch_bytes >= sparse_loss_scratch(), "sparse_loss_fwd: scratch too small (%zu < %zu)",
                scratch_bytes, sparse_loss_scratch());
  hipStream_t st = as_stream(stream);
  unsigned long long* wf = reinterpret_cast<unsigned long long*>(w_fix);
  PNR_HIP(hipMemsetAsync(wf, 0, (size_t)N * sizeof(unsigned long long), st));
  if (R > 0) {
    SparseArgs a = {R, N, R * q->SR, q->SR, q->K, b->n_filled, b->ray_off, b->ray_vcnt, b->pidx, b->sample_w,
                    xyz, wf};
    hipLaunchKernelGGL(k_sparse_weights, dim3(grid_for(R * 64, 256, 256 * 16)), dim3(256), 0, st, a);
    PNR_LAUNCH_CHECK();
  }
  double* pnum = static_cast<double*>(scratch);
  unsigned long long* pw = reinterpret_cast<unsigned long long*>(pnum + kLossBlocks);
  hipLaunchKernelGGL(k_sparse_part, dim3(kLossBlocks), dim3(256), 0, st, wf, conf, N, pnum, pw);
  PNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sparse_final, dim3(1), dim3(64), 0, st, pnum, pw, out, state);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_sparse_loss_bwd(const uint64_t* w_fix, const float* conf, int64_t N, const double* state,
                                   const float* g, float* d_conf, void* stream) {
  PNR_CHECK_ARG(w_fix && conf && state && g && d_conf, "sparse_loss_bwd: null pointer");
  PNR_CHECK_ARG(N > 0, "sparse_loss_bwd: N=%lld", (long long)N);
  PNR_CHECK_ARG(((uintptr_t)w_fix & 7) == 0 && ((uintptr_t)state & 7) == 0,
                "sparse_loss_bwd: w_fix and state must be 8-B aligned");
  hipLaunchKernelGGL(k_sparse_bwd, dim3(grid_for(N, 256, 2048)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(w_fix), conf, N, state, g, d_conf);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
