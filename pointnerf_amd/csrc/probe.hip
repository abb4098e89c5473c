// Point-growing probe (opt.prob == 1): per ray, the most opaque shading sample,
// its world location, the distance to its nearest gathered neighbour and the
// weight-averaged point attributes of that sample's K neighbours
// (neural_points_volumetric_model_ori.py:351-372, read by probe_hole,
// run/train_ft.py:473-515) -- straight from the query buffers and the
// composite's opacity[R,SR], in full ray order.  One wave per ray.
#include "pnr_common.h"

namespace pnr {

constexpr int kPBlock = 256;
constexpr int kProbeCh = 39;   // colour 3 + dir 3 + conf 1 + embedding 32

struct ProbeArgs {
  int64_t R;
  int SR, K;
  const int32_t* n_filled;
  const int32_t* ray_off;
  const int32_t* ray_vcnt;
  const int32_t* pidx;
  const float* sample_w;
  const float* xyz;
  const float* color;
  const float* dir;
  const float* conf;
  const float* emb;
  const uint16_t* emb_h;
  const float* opacity;
  float* max_opacity;
  float* max_loc_w;
  float* far_dist;
  float* avg_color;
  float* avg_dir;
  float* avg_conf;
  float* avg_emb;
};

// Channel c of the probe's 39 averaged values: where point p's value is read
// (nullptr tables: no such output) and where ray r's average goes.
__device__ __forceinline__ float* probe_out(const ProbeArgs& a, int64_t r, int c) {
  if (c < 3) return a.avg_color ? a.avg_color + r * 3 + c : nullptr;
  if (c < 6) return a.avg_dir ? a.avg_dir + r * 3 + (c - 3) : nullptr;
  if (c < 7) return a.avg_conf ? a.avg_conf + r : nullptr;
  return a.avg_emb + r * 32 + (c - 7);
}

// The raw 32 bits of point p's channel c: a float's, or a bf16's in the low half
// (probe_val turns them into the value once the load has landed).
__device__ __forceinline__ uint32_t probe_in(const ProbeArgs& a, int64_t p, int c) {
  if (c < 3) return __float_as_uint(a.color[p * 3 + c]);
  if (c < 6) return __float_as_uint(a.dir[p * 3 + (c - 3)]);
  if (c < 7) return __float_as_uint(a.conf[p]);
  if (a.emb_h) return a.emb_h[p * 32 + (c - 7)];
  return __float_as_uint(a.emb[p * 32 + (c - 7)]);
}

__device__ __forceinline__ float probe_val(const ProbeArgs& a, uint32_t bits, int c) {
  return __uint_as_float(c >= 7 && a.emb_h ? bits << 16 : bits);
}

__global__ void __launch_bounds__(kPBlock) k_probe(ProbeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int SR = a.SR, K = a.K;
  for (int64_t r = wave0; r < a.R; r += nwaves) {
    float* const out = lane < kProbeCh ? probe_out(a, r, lane) : nullptr;
    const int vcnt = a.ray_vcnt[r], n = a.n_filled[r], off = a.ray_off[r];   // one round trip, not three
    if (vcnt <= 0) {   // ray_mask == 0: an all-zero row
      if (lane == 0) {
        a.max_opacity[r] = 0.f;
        a.far_dist[r] = 0.f;
      }
      if (lane < 3) a.max_loc_w[r * 3 + lane] = 0.f;
      if (out) *out = 0.f;
      continue;
    }
    // s* = argmax_s opacity[r, s], the lowest slot among equal maxima
    float v = lane < SR ? a.opacity[r * SR + lane] : -INFINITY;
    int s = lane;
    if (lane + 64 < SR) {
      const float v1 = a.opacity[r * SR + lane + 64];
      if (v1 > v) {
        v = v1;
        s = lane + 64;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o);
      const int os = __shfl_xor(s, o);
      if (ov > v || (ov == v && os < s)) {
        v = ov;
        s = os;
      }
    }
    v = __shfl(v, 0);
    s = min(__shfl(s, 0), SR - 1);
    const bool filled = s < n;
    const int64_t i = (int64_t)off + s;   // read only when filled
    float sw[3] = {0.f, 0.f, 0.f};
    if (filled) {
      sw[0] = a.sample_w[i * 3];
      sw[1] = a.sample_w[i * 3 + 1];
      sw[2] = a.sample_w[i * 3 + 2];
    }
    // lane k < K: neighbour k of slot s*; an empty slot gathers point 0
    // (neural_points.py:790) for the distance and the averages, with weight 0
    int32_t pc = 0;
    float dist = INFINITY, wl = 0.f;
    if (lane < K) {
      const int32_t p = filled ? a.pidx[i * K + lane] : -1;
      pc = p > 0 ? p : 0;
      const float d0 = a.xyz[(int64_t)pc * 3] - sw[0], d1 = a.xyz[(int64_t)pc * 3 + 1] - sw[1],
                  d2 = a.xyz[(int64_t)pc * 3 + 2] - sw[2];
      dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      if (p >= 0) wl = 1.f / fmaxf(dist, 1e-6f);   // k_march_aux's weight, term by term
    }
    float fd = dist;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) fd = fminf(fd, __shfl_xor(fd, o));   // K <= 16
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += __shfl(wl, k);   // k_march_aux's order
    float wk = wl / fmaxf(sum, 1e-8f);
    if (lane < K && a.conf) wk *= fminf(fmaxf(a.conf[pc], 1e-4f), 1.f);
    // all K gathers of the lane's channel in flight before the first is used
    // (lanes >= K hold point 0 with weight 0 and are not read)
    uint32_t x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int32_t pk = __shfl(pc, k);
      x[k] = (out && k < K) ? probe_in(a, pk, lane) : 0u;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float w = __shfl(wk, k);
      if (k < K) acc += probe_val(a, x[k], lane) * w;
    }
    if (lane == 0) {
      a.max_opacity[r] = v;
      a.far_dist[r] = fd;
    }
    if (lane < 3) a.max_loc_w[r * 3 + lane] = sw[lane];
    if (out) *out = acc;
  }
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_probe(const pnr_rays* rays, const pnr_query_params* q, const pnr_query_bufs* b,
                         const pnr_points* pts, const float* opacity, float* max_opacity, float* max_loc_w,
                         float* far_dist, float* avg_color, float* avg_dir, float* avg_conf, float* avg_emb,
                         void* stream) {
  PNR_CHECK_ARG(rays && q && b && pts && opacity && max_opacity && max_loc_w && far_dist && avg_emb,
                "probe: null pointer");
  PNR_CHECK_ARG(pts->emb_dim == 0 || pts->emb_dim == 32,
                "probe: pnr_points.emb_dim (point_features_dim) must be 0 or 32 here");
  PNR_CHECK_ARG(q->SR >= 1 && q->SR <= 128, "probe: SR=%d unsupported (1..128)", q->SR);
  PNR_CHECK_ARG(q->K >= 1 && q->K <= 16, "probe: K=%d unsupported (1..16)", q->K);
  PNR_CHECK_ARG(b->n_filled && b->ray_off && b->ray_vcnt && b->pidx && b->sample_w, "probe: null query buffer");
  PNR_CHECK_ARG(pts->xyz && (pts->emb || pts->emb_bf16), "probe: xyz and an embedding table required");
  PNR_CHECK_ARG((!avg_color || pts->color) && (!avg_dir || pts->dir) && (!avg_conf || pts->conf),
                "probe: an average was asked of an absent point table");
  if (rays->R == 0) return PNR_OK;
  ProbeArgs a = {rays->R, q->SR, q->K, b->n_filled, b->ray_off, b->ray_vcnt, b->pidx, b->sample_w,
                 pts->xyz, pts->color, pts->dir, pts->conf, pts->emb, pts->emb_bf16, opacity,
                 max_opacity, max_loc_w, far_dist, avg_color, avg_dir, avg_conf, avg_emb};
  const unsigned grid = grid_for(rays->R * 64, kPBlock, 256 * 16);
  hipLaunchKernelGGL(k_probe, dim3(grid), dim3(kPBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
