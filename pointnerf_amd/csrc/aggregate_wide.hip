// The DTU aggregator configuration: embedding tables of
// any width E in 1..64 (pnr_points.emb_dim; the reference's DTU scripts use 63)
// and agg_intrp_order 1 (pnr_mlp.intrp_order).
//
// block1.0 splits exactly into a per-point half P1[p] = W1[:, :7E] .
// [emb_p, PE_3(emb_p)] + b1 and a per-pair distance half; the pair and colour
// kernels read P1 rows and never see the embedding, so a wider table only needs
// its own per-point pass:
//   * k_point_pre_w: k_point_pre (aggregate.hip) for a runtime E, on the same
//     fp32 MFMA layer, in accumulating K passes of at most 288 input rows so a
//     wave's LDS slice keeps k_point_pre's 296 rows (four waves, 153 KB);
//   * k_point_pre_h2_w (aggregate_x3.hip, beside k_point_pre_h2 and its `layer`
//     machinery): the f16-split counterpart.
// Order 1 is the order-2 chain with another tail (point_aggregators.py:573-599):
//   * k_tail_o1, after the colour kernel: alpha from the K-summed block3
//     features (the `hid` rows the colour kernels consume) and raw2out_color on
//     the colour branch's outputs.
// A row of E floats is only 4-B aligned when E % 4 != 0: every access to emb
// here is a dword load.
#include "agg_quad.h"

namespace pnr {
namespace {

constexpr int kWPitch = 33;                    // LDS row pitch (floats) of X^T[k][32 + 1], as k_point_pre
constexpr int kWSteps = 144;                   // k-steps (2 input rows each) per pass
constexpr int kWRows = 2 * kWSteps + 8;        // + the layer's B-operand prefetch overrun
constexpr int kWWaveLds = kWRows * kWPitch;    // floats per wave slice
constexpr size_t kWLdsBytes = (size_t)4 * kWWaveLds * sizeof(float);
static_assert(kWLdsBytes <= 160 * 1024, "LDS budget");

struct P1WArgs {
  pnr_points pts;
  const float* w1af;   // frag_pack of block1.0[:, :7E] + bias
  float* p1;           // [n_p1, 256]
  int E;
};

template <int NT>
__device__ __forceinline__ void mfma_step_w(f32x16 (&acc)[NT], const float (&a)[NT], float x) {
#pragma unroll
  for (int T = 0; T < NT; ++T) acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[T], x, acc[T], 0, 0, 0);
}

// acc += W[:, 2 t0 ..] . X^T over nsteps k-steps: the layer loop of k_point_pre
// (weights four k-steps ahead, B operands one iteration ahead) starting at
// k-step t0 of the pack; X^T row 0 is input row 2 t0.  The pack's zero steps
// (kPackPad) and the slice's 8 spare rows take the prefetch overrun.
__device__ __forceinline__ void layer_w(f32x16 (&acc)[8], const float* __restrict__ wf, int t0, const float* X,
                                        int nsteps, int lane) {
  constexpr int NT = 8, D = 4;
  const int m = lane & 31, h = lane >> 5;
  const float* p = wf + (size_t)t0 * NT * 64 + lane;
  const float* xr = X + h * kWPitch + m;
  float a0[NT], a1[NT], a2[NT], a3[NT];
  load_w<NT>(a0, p, 0);
  load_w<NT>(a1, p, 1);
  load_w<NT>(a2, p, 2);
  load_w<NT>(a3, p, 3);
  float x0 = xr[0], x1 = xr[2 * kWPitch], x2 = xr[4 * kWPitch], x3 = xr[6 * kWPitch];
  int t = 0;
#pragma unroll 1
  for (; t + D <= nsteps; t += D) {
    const float* xn = xr + 2 * (t + D) * kWPitch;
    mfma_step_w<NT>(acc, a0, x0);
    const float y0 = xn[0], y1 = xn[2 * kWPitch], y2 = xn[4 * kWPitch], y3 = xn[6 * kWPitch];
    load_w<NT>(a0, p, t + 4);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step_w<NT>(acc, a1, x1);
    load_w<NT>(a1, p, t + 5);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step_w<NT>(acc, a2, x2);
    load_w<NT>(a2, p, t + 6);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step_w<NT>(acc, a3, x3);
    load_w<NT>(a3, p, t + 7);
    __builtin_amdgcn_sched_barrier(0);
    x0 = y0;
    x1 = y1;
    x2 = y2;
    x3 = y3;
  }
  const int rem = nsteps - t;  // 0..3
  if (rem > 0) mfma_step_w<NT>(acc, a0, x0);
  if (rem > 1) mfma_step_w<NT>(acc, a1, x1);
  if (rem > 2) mfma_step_w<NT>(acc, a2, x2);
}

// Input rows in the reference's order (networks.py:175-190): 0..E-1 the
// embedding, E + 6c + {s0, c0, s1, c1, s2, c2} the PE of channel c (angle
// doubling from one sincos, as k_point_pre: both widths round alike), 7E the
// bias column's 1, 7E + 1 a zero when the last k-step is shared.
__global__ void __launch_bounds__(kAggBlock, 1) k_point_pre_w(P1WArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds_w[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* X = lds_w + wid * kWWaveLds;
  const int m = lane & 31, h = lane >> 5;
  const int E = A.E;
  const int rows = 7 * E + 1;               // inputs + bias
  const int steps = (rows + 1) >> 1;
  const int64_t np = p1_rows(A.pts);   // P1 rows
  const int64_t ntiles = cdiv(np, 32);
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wid; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t pt = tile * 32 + m;                         // P1 row
    const bool act = pt < np;
    const int64_t prow = act ? (A.pts.used ? (int64_t)A.pts.used[pt] : pt) : 0;   // point row
    const float* e = A.pts.emb + prow * E;
    f32x16 acc[8];
#pragma unroll
    for (int T = 0; T < 8; ++T) acc[T] = (f32x16){0.f};
    for (int t0 = 0; t0 < steps; t0 += kWSteps) {
      const int ns = steps - t0 < kWSteps ? steps - t0 : kWSteps;
      const int r0 = 2 * t0, r1 = r0 + 2 * ns;   // this pass: input rows [r0, r1)
      // lane half h owns the channels c = h (mod 2) that have a row in the pass
#pragma unroll 1
      for (int c = h; c < E; c += 2) {
        const int pe0 = E + 6 * c;
        const bool own = c >= r0 && c < r1;
        if (!own && (pe0 + 6 <= r0 || pe0 >= r1)) continue;
        const float ev = act ? e[c] : 0.f;
        if (own) X[(c - r0) * kWPitch + m] = ev;
        float s0, c0;
        sincosf(ev, &s0, &c0);
        const float s1 = 2.f * s0 * c0, c1 = (c0 - s0) * (c0 + s0);
        const float s2 = 2.f * s1 * c1, c2 = (c1 - s1) * (c1 + s1);
        const float pe[6] = {s0, c0, s1, c1, s2, c2};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const int r = pe0 + j;
          if (r >= r0 && r < r1) X[(r - r0) * kWPitch + m] = pe[j];
        }
      }
      if (h == 0 && rows - 1 >= r0 && rows - 1 < r1) X[(rows - 1 - r0) * kWPitch + m] = 1.f;
      if (h == 1 && rows >= r0 && rows < r1) X[(rows - r0) * kWPitch + m] = 0.f;
      wave_sync();
      layer_w(acc, A.w1af, t0, X, ns, lane);
      wave_sync();
    }
    if (act) {
      float4* o = reinterpret_cast<float4*>(A.p1 + pt * kHid);
#pragma unroll
      for (int T = 0; T < 8; ++T)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[8 * T + 2 * q + h] = make_float4(acc[T][4 * q], acc[T][4 * q + 1], acc[T][4 * q + 2], acc[T][4 * q + 3]);
    }
  }
}

// ---------------------------------------------------------------------------
// Order-1 tail.  One wave per list entry v < min(*n_dev, n_max) with a valid
// neighbour (vmask): out_feat[v, 0] = raw2out_density(wa . hid_v + ba),
// overwriting the K-summed per-pair alpha the pair kernel left there, and
// out_feat[v, 1..128] = raw2out_color of what the colour kernel wrote.  Every
// other row stays untouched.  hid: fp32 rows [n_max][256], or (planes) the
// f16-split planes k_pairs_h2 leaves for k_color_h2 -- per 64-sample tile
// [2 planes][32 row groups][64 samples][8 f16], x = xh + 2^-11 xl, the value
// k_color_h2 multiplies (aggregate_x3.hip, kHidTile).
constexpr int kTailHidPlane = 32 * 64 * 16;
constexpr int kTailHidTile = 2 * kTailHidPlane;

struct TailArgs {
  pnr_samples s;
  const float* hid;
  const int32_t* vmask;
  const float* wa;
  const float* ba;
  float* out_feat;
  int act_super;
  int planes;
};

__global__ void __launch_bounds__(256) k_tail_o1(TailArgs A) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int64_t n = eff_n(A.s);
  float w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = A.wa[4 * lane + i];
  const float ba = A.ba[0];
  for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += (int64_t)gridDim.x * 4) {
    if (A.vmask[v] == 0) continue;
    float x[4];   // hid_v[4 lane .. 4 lane + 3]
    if (A.planes) {
      const char* base = reinterpret_cast<const char*>(A.hid) + (v >> 6) * kTailHidTile +
                         (((lane >> 1) * 64 + (v & 63)) * 16 + 8 * (lane & 1));
      const h4 a = *reinterpret_cast<const h4*>(base), b = *reinterpret_cast<const h4*>(base + kTailHidPlane);
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = fmaf((float)b[i], 1.f / 2048.f, (float)a[i]);
    } else {
      const float4 r = reinterpret_cast<const float4*>(A.hid + v * kHid)[lane];
      x[0] = r.x; x[1] = r.y; x[2] = r.z; x[3] = r.w;
    }
    float d = fmaf(x[3], w[3], fmaf(x[2], w[2], fmaf(x[1], w[1], x[0] * w[0])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    float* of = A.out_feat + v * (kC + 1);
    if (lane == 0) {
      const float pa = d + ba;
      of[0] = A.act_super ? softplus(pa - 1.f) : fmaxf(pa, 0.f);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float c = 1.f / (1.f + expf(-of[1 + 64 * j + lane]));   // torch.sigmoid
      of[1 + 64 * j + lane] = A.act_super ? c * 1.002f - 0.001f : c;
    }
  }
}

}  // namespace

int launch_point_pre_w(const pnr_points& pts, const float* w1af, float* p1, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    PNR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_point_pre_w),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWLdsBytes));
    attr = true;
  }
  P1WArgs a;
  a.pts = pts;
  a.w1af = w1af;
  a.p1 = p1;
  a.E = emb_width(pts);
  hipLaunchKernelGGL(k_point_pre_w, dim3(grid_for(cdiv(pts.used ? pts.n_used : pts.n, 32), 4, 256)),
                     dim3(kAggBlock), kWLdsBytes, st, a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

int launch_tail_o1(const pnr_samples& s, const pnr_mlp& w, const float* hid, bool planes, const int32_t* vmask,
                   float* out_feat, hipStream_t st) {
  TailArgs a;
  a.s = s;
  a.hid = hid;
  a.vmask = vmask;
  a.wa = w.wa;
  a.ba = w.ba;
  a.out_feat = out_feat;
  a.act_super = w.act_super;
  a.planes = planes ? 1 : 0;
  hipLaunchKernelGGL(k_tail_o1, dim3(grid_for(s.n_max, 4, 256 * 8)), dim3(256), 0, st, a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

}  // namespace pnr
