// The aggregate's backward: k_pairs_bwd<0|1|2> with its fp32x3 /
// fp32h2 split-MFMA dX layers, the block3.0 extras passes (k_extras_bwd,
// k_extras_rows) and d xyz (k_xyz_bwd), behind pnr_aggregate_bwd_pairs(_x3|_h2),
// pnr_aggregate_bwd_extras_rows and pnr_aggregate_bwd_xyz.  The forwards that
// save the activations read here are in aggregate.hip and aggregate_x3.hip.
#include "agg_quad.h"

namespace pnr {

// k_pairs_bwd mirrors k_pairs (aggregate.hip): a 4-wave workgroup
// owns 64 pairs, wave w owns neuron tiles {2w, 2w+1} of both halves, and the
// three dX GEMMs (block3.2^T, block3.0[:, :256]^T, block1.2^T) run on the same
// quad-row LDS pipeline with transposed, fragment-packed weights.  The dW
// GEMMs (sum over pairs) are plain GEMMs and left to the caller (hipBLASLt).
struct BwdArgs {
  pnr_points pts;
  pnr_samples s;
  pnr_mlp w;
  pnr_mlp_bwd wb;
  pnr_agg_saved sv;
  const float* d_feat;   // [n,129]
  const float* d_hid;    // [n,256]
  float* dz[4];          // dz1..dz4 [n*8,256]
  float* dpa;            // [n*8]
  float* d_p1;           // [N,256] (+=)
  float* d_color;        // [N,3] (+=) or null
  float* d_dir;          // [N,3] (+=) or null
  float* d_conf;         // [n*8] per pair (written; summed per point by pnr_pairs_to_points_conf) or null
  const void* wx[3];     // k_pairs_bwd<1>: frag_pack_x3 of W4^T, W3[:, :256]^T, W2^T;
                         // k_pairs_bwd<2>: the three pnr_pack_bwd_h2 packs
  const float* wxs;      // k_pairs_bwd<2>: device [3], the packs' scales 2^(s - 11)
};

constexpr int kBwdLdsFloats = 66 * kQP + 4 * kTP /*dot parts*/ + 4 * 7 * kTP /*extras parts*/;
constexpr size_t kBwdLdsBytes = (size_t)kBwdLdsFloats * sizeof(float);

// acc-layout float4 of a [pair][256] array for (half pt, tile T, quad q)
__device__ __forceinline__ float4 ld_q(const float* base, int64_t pair, int T, int q, int h) {
  return *reinterpret_cast<const float4*>(base + pair * kHid + 32 * T + 8 * q + 4 * h);
}

// Raw (no activation) accumulator quads -> quad rows.
template <int NT, int PT>
__device__ __forceinline__ void store_q(const f32x16 (&acc)[PT * NT], float* X, int lane, int T0) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x16& v = acc[pt * NT + T];
        *reinterpret_cast<float4*>(X + (8 * (T0 + T) + 2 * q + h) * kQP + 4 * (32 * pt + c)) =
            make_float4(v[4 * q], v[4 * q + 2], v[4 * q + 1], v[4 * q + 3]);
      }
}

// dz = dh * lrelu'(h) with h the saved post-activation (h > 0 <=> z > 0 for
// slope >= 0); writes dz back into acc and to dst rows of active pairs.
template <int NT, int PT>
__device__ __forceinline__ void lrelu_bwd_q(f32x16 (&acc)[PT * NT], const float* h_saved, float* dst,
                                            int64_t tile, int64_t n, float slope, int lane, int T0,
                                            unsigned* amx = nullptr) {
  const int c = lane & 31, h = lane >> 5;
  unsigned mb = 0;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int col = 32 * pt + c;
    const bool act = tile * kTS + (col >> 3) < n;
    const int64_t pair = tile * kTP + col;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x16& v = acc[pt * NT + T];
        float4 hv = act ? ld_q(h_saved, pair, T0 + T, q, h) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * q + 0] = hv.x > 0.f ? v[4 * q + 0] : v[4 * q + 0] * slope;
        v[4 * q + 1] = hv.y > 0.f ? v[4 * q + 1] : v[4 * q + 1] * slope;
        v[4 * q + 2] = hv.z > 0.f ? v[4 * q + 2] : v[4 * q + 2] * slope;
        v[4 * q + 3] = hv.w > 0.f ? v[4 * q + 3] : v[4 * q + 3] * slope;
        if (!act) v[4 * q] = v[4 * q + 1] = v[4 * q + 2] = v[4 * q + 3] = 0.f;
        if (act)
          *reinterpret_cast<float4*>(dst + pair * kHid + 32 * (T0 + T) + 8 * q + 4 * h) =
              make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        if (amx) {
#pragma unroll
          for (int i = 0; i < 4; ++i) mb = max(mb, __float_as_uint(fabsf(v[4 * q + i])));
        }
      }
  }
  if (amx) wave_absmax_to(amx, mb);
}

// dz = dh * lrelu'(z) from the saved derivative bits (words prefetched by
// load_masks before the layer's GEMM, so the mask latency hides behind it).
template <int NT, int PT>
__device__ __forceinline__ void load_masks(unsigned (&mk)[PT * NT], const uint16_t* mask, int layer, int64_t tile,
                                           int64_t n, int lane, int T0) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int col = 32 * pt + c;
    const bool act = tile * kTS + (col >> 3) < n;
#pragma unroll
    for (int T = 0; T < NT; ++T)
      mk[pt * NT + T] = act ? mask[(tile * kTP + col) * 64 + 16 * layer + 2 * (T0 + T) + h] : 0u;
  }
}

template <int NT, int PT>
__device__ __forceinline__ void lrelu_bwd_m(f32x16 (&acc)[PT * NT], const unsigned (&mk)[PT * NT], float* dst,
                                            int64_t tile, int64_t n, float slope, int lane, int T0,
                                            unsigned* amx = nullptr) {
  const int c = lane & 31, h = lane >> 5;
  unsigned mb = 0;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int col = 32 * pt + c;
    const bool act = tile * kTS + (col >> 3) < n;
    const int64_t pair = tile * kTP + col;
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      f32x16& v = acc[pt * NT + T];
      const unsigned b = mk[pt * NT + T];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = act ? (((b >> r) & 1u) ? v[r] : v[r] * slope) : 0.f;
      if (act) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(dst + pair * kHid + 32 * (T0 + T) + 8 * q + 4 * h) =
              make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
      }
      if (amx) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mb = max(mb, __float_as_uint(fabsf(v[r])));
      }
    }
  }
  if (amx) wave_absmax_to(amx, mb);
}

// ---- fp32x3 dX GEMMs of k_pairs_bwd<true>: the transposed weights as exact
// 3-way bf16 splits (frag_pack_x3: F[t][T][plane][lane][8], X3_PAD zero steps),
// the B fragments read from the fp32 quad rows and split into three bf16
// planes in registers (split2, exact), six cross products per 16-k step on
// v_mfma_f32_32x32x16_bf16 (smallest first) -- the arithmetic of the fp32x3
// forward (aggregate_x3.hip) on k_pairs_bwd's LDS layout.
constexpr int kX3D = 3;   // weight ring depth (k-steps in flight) <= X3_PAD
struct X3QRing {
  uint4 a[kX3D][2][3];
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t x3q_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

// this wave's two neuron tiles of k-step t, three planes each; voff = (T0 * 3 * 64 + lane) * 16
__device__ __forceinline__ void x3q_load(uint4 (&a)[2][3], __amdgpu_buffer_rsrc_t rs, int voff, int t) {
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      a[T][pl] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + pl * 1024,
                                                                                   (t * 8 + T) * 3 * 1024, 0));
}

__device__ __forceinline__ void x3q_prime(X3QRing& w, __amdgpu_buffer_rsrc_t rs, int voff) {
#pragma unroll
  for (int d = 0; d < kX3D; ++d) x3q_load(w.a[d], rs, voff, d);
}

// B fragment of k-step t, pair half pt: inputs 16t + 8h .. +7 of pair 32pt + c
// (quad rows 4t + 2h, 4t + 2h + 1; each float4 holds neurons (0, 2, 1, 3))
__device__ __forceinline__ void x3q_b(const float* X, int t, int pt, int lane, uint4 (&b)[3]) {
  const int c = lane & 31, h = lane >> 5;
  const float* xb = X + (4 * t + 2 * h) * kQP + 4 * (32 * pt + c);
  const float4 q0 = *reinterpret_cast<const float4*>(xb);
  const float4 q1 = *reinterpret_cast<const float4*>(xb + kQP);
  unsigned w0[4], w1[4], w2[4];
  split2(q0.x, q0.z, w0[0], w1[0], w2[0]);
  split2(q0.y, q0.w, w0[1], w1[1], w2[1]);
  split2(q1.x, q1.z, w0[2], w1[2], w2[2]);
  split2(q1.y, q1.w, w0[3], w1[3], w2[3]);
  b[0] = make_uint4(w0[0], w0[1], w0[2], w0[3]);
  b[1] = make_uint4(w1[0], w1[1], w1[2], w1[3]);
  b[2] = make_uint4(w2[0], w2[1], w2[2], w2[3]);
}

// acc[2 pt + T] += W^T . X over nsteps 16-k steps (weights kX3D steps ahead
// in the ring)
// (the ring is primed here, not ahead across the tile's other phases: 72 VGPRs
// live through the whole tile made the kernel spill)
__device__ __forceinline__ void mlp_layer_x3q(f32x16 (&acc)[4], __amdgpu_buffer_rsrc_t rs, int voff,
                                              const float* X, int nsteps, int lane) {
  X3QRing w;
  x3q_prime(w, rs, voff);
  uint4 b[2][3];
  x3q_b(X, 0, 0, lane, b[0]);
  x3q_b(X, 0, 1, lane, b[1]);
  auto step = [&](uint4 (&a)[2][3], int t) {
    if (t > 0) {
      x3q_b(X, t, 0, lane, b[0]);
      x3q_b(X, t, 1, lane, b[1]);
    }
    // products smallest first (W2.X0, W1.X1, W0.X2, W1.X0, W0.X1, W0.X0), each
    // over the four accumulators in turn: four independent MFMA chains
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int T = 0; T < 2; ++T) acc[2 * pt + T] = mfma_bf16(a[T][kPa[p]], b[pt][kPb[p]], acc[2 * pt + T]);
    x3q_load(a, rs, voff, t + kX3D);   // packs carry kX3D zero steps
  };
  int t = 0;
#pragma unroll 1
  for (; t + kX3D <= nsteps; t += kX3D) {
#pragma unroll
    for (int d = 0; d < kX3D; ++d) step(w.a[d], t + d);
  }
#pragma unroll
  for (int d = 0; d < kX3D - 1; ++d)
    if (t + d < nsteps) step(w.a[d], t + d);
}

// ---- fp32h2 dX GEMMs of k_pairs_bwd<2>: the transposed weights as f16 (hi,
// 2^11 lo) pairs of 2^-s W (pnr_pack_bwd_h2: F[t][T][plane][lane][8], kX3D zero
// steps), the B fragments split from the fp32 quad rows times the tile's power
// of two xs (max |X| xs in [2^13, 2^14): every value of the tile keeps 22
// significant bits down to 2^-14 of the maximum), three products per 16-k step
// on v_mfma_f32_32x32x16_f16 -- 2^11 (2^-s W X xs) in the accumulators, which
// the caller scales back.
struct H2QRing {
  uint4 a[kX3D][2][2];
};

__device__ __forceinline__ void h2q_load(uint4 (&a)[2][2], __amdgpu_buffer_rsrc_t rs, int voff, int t) {
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
      a[T][pl] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + pl * 1024,
                                                                                   (t * 8 + T) * 2 * 1024, 0));
}

__device__ __forceinline__ void h2q_b(const float* X, int t, int pt, int lane, float xs, uint4 (&b)[2]) {
  const int c = lane & 31, h = lane >> 5;
  const float* xb = X + (4 * t + 2 * h) * kQP + 4 * (32 * pt + c);
  const float4 q0 = *reinterpret_cast<const float4*>(xb);
  const float4 q1 = *reinterpret_cast<const float4*>(xb + kQP);
  unsigned w0[4], w1[4];
  splith(q0.x * xs, q0.z * xs, w0[0], w1[0]);
  splith(q0.y * xs, q0.w * xs, w0[1], w1[1]);
  splith(q1.x * xs, q1.z * xs, w0[2], w1[2]);
  splith(q1.y * xs, q1.w * xs, w0[3], w1[3]);
  b[0] = make_uint4(w0[0], w0[1], w0[2], w0[3]);
  b[1] = make_uint4(w1[0], w1[1], w1[2], w1[3]);
}

__device__ __forceinline__ void mlp_layer_h2q(f32x16 (&acc)[4], __amdgpu_buffer_rsrc_t rs, int voff,
                                              const float* X, int nsteps, int lane, float xs) {
  H2QRing w;
#pragma unroll
  for (int d = 0; d < kX3D; ++d) h2q_load(w.a[d], rs, voff, d);
  uint4 b[2][2];
  h2q_b(X, 0, 0, lane, xs, b[0]);
  h2q_b(X, 0, 1, lane, xs, b[1]);
  auto step = [&](uint4 (&a)[2][2], int t) {
    if (t > 0) {
      h2q_b(X, t, 0, lane, xs, b[0]);
      h2q_b(X, t, 1, lane, xs, b[1]);
    }
    // smallest terms first: Wl.Xh, Wh.Xl, then 2^11 Wh.Xh; four independent chains
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int T = 0; T < 2; ++T) acc[2 * pt + T] = mfma_f16(a[T][1], b[pt][0], acc[2 * pt + T]);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int T = 0; T < 2; ++T) acc[2 * pt + T] = mfma_f16(a[T][0], b[pt][1], acc[2 * pt + T]);
    const uint4 as0 = f16x8_scale2048(a[0][0]), as1 = f16x8_scale2048(a[1][0]);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      acc[2 * pt] = mfma_f16(as0, b[pt][0], acc[2 * pt]);
      acc[2 * pt + 1] = mfma_f16(as1, b[pt][0], acc[2 * pt + 1]);
    }
    h2q_load(a, rs, voff, t + kX3D);   // packs carry kX3D zero steps
  };
  int t = 0;
#pragma unroll 1
  for (; t + kX3D <= nsteps; t += kX3D) {
#pragma unroll
    for (int d = 0; d < kX3D; ++d) step(w.a[d], t + d);
  }
#pragma unroll
  for (int d = 0; d < kX3D - 1; ++d)
    if (t + d < nsteps) step(w.a[d], t + d);
}

// max |v| over this wave's accumulators into slot (one float per wave; NaN as +inf)
__device__ __forceinline__ void wave_tile_absmax(const f32x16 (&acc)[4], float* slot) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = fabsf(acc[i][r]);
      m = a != a ? __builtin_inff() : fmaxf(m, a);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) *slot = m;
}

// the tile's X factor xs = 2^e (max |X| xs in [2^13, 2^14), e <= 126) from the
// four waves' maxima; 1 for an all-zero or non-finite tile
__device__ __forceinline__ float tile_xscale(const float* slots) {
  const float m = fmaxf(fmaxf(slots[0], slots[1]), fmaxf(slots[2], slots[3]));
  if (!(m > 0.f) || !(m <= 3.0e38f)) return 1.f;
  int E;
  (void)frexpf(m, &E);   // m = f 2^E, f in [0.5, 1)
  return ldexpf(1.f, min(14 - E, 126));
}

// acc = acc / xs * ws (two steps: each factor alone stays in the normal range)
__device__ __forceinline__ void h2q_unscale(f32x16 (&acc)[4], float xs, float ws) {
  const float xu = 1.f / xs;   // exact: xs is a power of two
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = (acc[i][r] * xu) * ws;
}


// V = 0: native fp32 dX GEMMs; 1: fp32x3 (split bf16); 2: fp32h2 (split f16,
// per-tile power-of-two scaling of X).  V >= 1 leaves the block3.0 extras to a
// separate pass.
template <int V>
__global__ void __launch_bounds__(64 * kPairWaves, 2) k_pairs_bwd(BwdArgs A) {
  constexpr bool X3 = V != 0;
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  float* X = lds_dyn;                   // quad rows [66][kQP]
  float* dotp = X + 66 * kQP;           // [4][64] partial <d_hid, h4> per wave
  float* exP = dotp + 4 * kTP;          // [4][7][64] partial block3.0 extras gradients (V == 0)
  float* tmx = exP;                     // [4] per-wave max |X| of the layer input (V == 2)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int j = lane >> 3;
  const int T0 = wid * kNTW;
  const int64_t n = eff_n(A.s);
  const int64_t ntiles = cdiv(n, kTS);
  const float slope = A.w.neg_slope;
  const float* w4t = X3 ? nullptr : A.wb.w4t + T0 * 64;
  const float* w3t = X3 ? nullptr : A.wb.w3t + T0 * 64;
  const float* w2t = X3 ? nullptr : A.wb.w2t + T0 * 64;
  float ring[kQD][kNTW];
  const int xvoff = (T0 * (V == 2 ? 2 : 3) * 64 + lane) * 16;
  const __amdgpu_buffer_rsrc_t x4 = x3q_rsrc(A.wx[0]), x3 = x3q_rsrc(A.wx[1]), x2 = x3q_rsrc(A.wx[2]);
  const float ws4 = V == 2 ? A.wxs[0] : 1.f, ws3 = V == 2 ? A.wxs[1] : 1.f, ws2 = V == 2 ? A.wxs[2] : 1.f;
  if constexpr (!X3) prime_q<kNTW>(ring, w4t, lane);
  // max |dz1..dz4|, |dpa| of this workgroup (pnr_agg_saved.dz_absmax: pnr_gemm_tn_h2's scales)
  __shared__ unsigned amx[5];
  unsigned* const am = A.sv.dz_absmax ? amx : nullptr;
  if (threadIdx.x < 5) amx[threadIdx.x] = 0u;
  __syncthreads();

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---------------------------------------------------------- per-pair scalars (lane = pair)
    const int64_t v = tile * kTS + j;
    const bool active = v < n;
    const int64_t pair = tile * kTP + lane;
    const bool svalid = active && A.sv.vmask[v] != 0;
    const float wt = active ? A.sv.wt[pair] : 0.f;
    const float pa = active ? A.sv.pa[pair] : 0.f;
    const float dalpha = svalid ? A.d_feat[v * (kC + 1)] : 0.f;
    // alpha_k = softplus(pa - 1) (threshold 20) or relu(pa) (point_aggregators.py:262-267)
    float a_k, sig;
    if (A.w.act_super) {
      const float x = pa - 1.f;
      a_k = softplus(x);
      sig = x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
    } else {
      a_k = fmaxf(pa, 0.f);
      sig = pa > 0.f ? 1.f : 0.f;
    }
    const float dpa = dalpha * wt * sig;   // d alpha_s / d pa_k
    if (wid == 0 && active) A.dpa[pair] = dpa;
    if (am && wid == 0) wave_absmax_to(am + 4, active ? __float_as_uint(fabsf(dpa)) : 0u);
    // ---------------------------------------------------------- d h4 -> dz4 (acc layout)
    f32x16 acc[kPTW * kNTW];
    float dot[kPTW];
#pragma unroll
    for (int pt = 0; pt < kPTW; ++pt) {
      const int col = 32 * pt + c;
      const int64_t pp = tile * kTP + col;
      const int64_t vv = tile * kTS + (col >> 3);
      const bool act = vv < n;
      const float wt_p = __shfl(wt, col), dpa_p = __shfl(dpa, col);
      const bool sv_p = __shfl((int)svalid, col) != 0;
      dot[pt] = 0.f;
#pragma unroll
      for (int T = 0; T < kNTW; ++T)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 h4 = act ? ld_q(A.sv.h4, pp, T0 + T, q, h) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 df = sv_p ? ld_q(A.d_hid, vv, T0 + T, q, h) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 wa = *reinterpret_cast<const float4*>(A.w.wa + 32 * (T0 + T) + 8 * q + 4 * h);
          dot[pt] += df.x * h4.x + df.y * h4.y + df.z * h4.z + df.w * h4.w;
          // f_s = sum_k wt_k h4_k ; alpha_s = sum_k wt_k softplus(wa.h4_k + ba - 1)
          acc[pt * kNTW + T][4 * q + 0] = wt_p * df.x + dpa_p * wa.x;
          acc[pt * kNTW + T][4 * q + 1] = wt_p * df.y + dpa_p * wa.y;
          acc[pt * kNTW + T][4 * q + 2] = wt_p * df.z + dpa_p * wa.z;
          acc[pt * kNTW + T][4 * q + 3] = wt_p * df.w + dpa_p * wa.w;
        }
      dot[pt] += __shfl_xor(dot[pt], 32);
    }
    if (h == 0) {
      dotp[wid * kTP + c] = dot[0];
      dotp[wid * kTP + 32 + c] = dot[1];
    }
    lrelu_bwd_q<kNTW, kPTW>(acc, A.sv.h4, A.dz[3], tile, n, slope, lane, T0, am ? am + 3 : nullptr);
    store_q<kNTW, kPTW>(acc, X, lane, T0);
    if constexpr (V == 2) wave_tile_absmax(acc, tmx + wid);
    __syncthreads();
    // d wt_k = d alpha_s a_k + <d f_s, h4_k>  ->  d conf_k (straight-through clamp, :724-726)
    // One term per pair, written: the per-point sums follow in pair order
    // (pnr_pairs_to_points_conf), so d conf does not depend on the order the waves arrive in.
    if (wid == 0 && active && A.d_conf) {
      const int32_t pr = A.sv.prow[pair];
      float dc = 0.f;
      if (pr >= 0) {
        const float dwt = dalpha * a_k + dotp[lane] + dotp[kTP + lane] + dotp[2 * kTP + lane] +
                          dotp[3 * kTP + lane];
        dc = dwt * A.sv.wn[pair];
      }
      A.d_conf[pair] = dc;
    }
    // ---------------------------------------------------------- block3.2^T: dh3 = W4^T dz4
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    unsigned mk[kPTW * kNTW];
    load_masks<kNTW, kPTW>(mk, A.sv.mask, 2, tile, n, lane, T0);
    if constexpr (V == 2) {
      const float xs = tile_xscale(tmx);
      mlp_layer_h2q(acc, x4, xvoff, X, 16, lane, xs);
      h2q_unscale(acc, xs, ws4);
    } else if constexpr (X3) {
      mlp_layer_x3q(acc, x4, xvoff, X, 16, lane);
    } else {
      mlp_layer_q<kNTW, kPTW>(acc, ring, w4t, X, 128, lane);
      prime_q<kNTW>(ring, w3t, lane);
    }
    __syncthreads();
    lrelu_bwd_m<kNTW, kPTW>(acc, mk, A.dz[2], tile, n, slope, lane, T0, am ? am + 2 : nullptr);
    store_q<kNTW, kPTW>(acc, X, lane, T0);
    if constexpr (V == 2) wave_tile_absmax(acc, tmx + wid);
    // block3.0 extras (inputs 256..262): d x3e_e = sum_n W3[n, 256 + e] dz3[n];
    // wave w reads back its own 64 dz3 rows (quad rows 16w..16w+15), lane = pair
    wave_sync();
    if constexpr (!X3) {
      float ex[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int u = 16 * wid; u < 16 * wid + 16; ++u) {
        const float4 x4 = *reinterpret_cast<const float4*>(X + u * kQP + 4 * lane);
        const float xv[4] = {x4.x, x4.z, x4.y, x4.w};   // neurons 4u + 0..3 (quad perm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float* we = A.wb.w3e + (4 * u + i) * 7;
#pragma unroll
          for (int e = 0; e < 7; ++e) ex[e] += we[e] * xv[i];
        }
      }
#pragma unroll
      for (int e = 0; e < 7; ++e) exP[(wid * 7 + e) * kTP + lane] = ex[e];
    }
    __syncthreads();
    // colour / dir gradients of the pair (wave 0, lane = pair), before the
    // block3.0^T GEMM: its registers stay free for the GEMM.  The pair's
    // indices are recomputed here rather than kept live across the GEMMs.
    if (!X3 && wid == 0 && tile * kTS + (lane >> 3) < n) {
      const int64_t pair = tile * kTP + lane;
      const int64_t v = tile * kTS + (lane >> 3);
      const int32_t pr = A.sv.prow[pair];
      if (pr >= 0) {
        float g[7];
#pragma unroll
        for (int e = 0; e < 7; ++e)
          g[e] = exP[(0 * 7 + e) * kTP + lane] + exP[(1 * 7 + e) * kTP + lane] + exP[(2 * 7 + e) * kTP + lane] +
                 exP[(3 * 7 + e) * kTP + lane];
        if (A.d_color) {
#pragma unroll
          for (int a = 0; a < 3; ++a) atomicAdd(A.d_color + (int64_t)pr * 3 + a, g[a]);
        }
        if (A.d_dir) {
          // inputs: R.dir - R.v (3), <R.dir, R.v> (1) with R.dir = dir @ Rw^T
          const int64_t row = sample_row(A.s, v);
          const int64_t drow = dir_row(A.s, row);
          const float vd[3] = {A.s.dirs[drow * 3], A.s.dirs[drow * 3 + 1], A.s.dirs[drow * 3 + 2]};
          float Rw[9];   // loaded here, not kept live across the tile's GEMMs
#pragma unroll
          for (int i = 0; i < 9; ++i) Rw[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
          float vrot[3];
          mat3(Rw, vd, vrot);
          if (A.pts.rw2c) {   // per-point: view dir by the slot-0 matrix, d dir through the pair's
            rot_point(A.pts.rw2c, slot0_point(A.s, row), vd, vrot);
#pragma unroll
            for (int i = 0; i < 9; ++i) Rw[i] = A.pts.rw2c[(int64_t)pr * 9 + i];
          }
          const float gd[3] = {g[3] + vrot[0] * g[6], g[4] + vrot[1] * g[6], g[5] + vrot[2] * g[6]};
          // drot_j = sum_i Rw[j][i] dir_i  ->  d dir_i = sum_j Rw[j][i] d drot_j
#pragma unroll
          for (int i = 0; i < 3; ++i)
            atomicAdd(A.d_dir + (int64_t)pr * 3 + i, Rw[i] * gd[0] + Rw[3 + i] * gd[1] + Rw[6 + i] * gd[2]);
        }
      }
    }
    // ---------------------------------------------------------- block3.0^T: dh2 = W3[:, :256]^T dz3
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    load_masks<kNTW, kPTW>(mk, A.sv.mask, 1, tile, n, lane, T0);
    if constexpr (V == 2) {
      const float xs = tile_xscale(tmx);
      mlp_layer_h2q(acc, x3, xvoff, X, 16, lane, xs);
      h2q_unscale(acc, xs, ws3);
    } else if constexpr (X3) {
      mlp_layer_x3q(acc, x3, xvoff, X, 16, lane);
    } else {
      mlp_layer_q<kNTW, kPTW>(acc, ring, w3t, X, 128, lane);
      prime_q<kNTW>(ring, w2t, lane);
    }
    __syncthreads();
    lrelu_bwd_m<kNTW, kPTW>(acc, mk, A.dz[1], tile, n, slope, lane, T0, am ? am + 1 : nullptr);
    store_q<kNTW, kPTW>(acc, X, lane, T0);
    if constexpr (V == 2) wave_tile_absmax(acc, tmx + wid);
    __syncthreads();
    // ---------------------------------------------------------- block1.2^T: dh1 = W2^T dz2
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    load_masks<kNTW, kPTW>(mk, A.sv.mask, 0, tile, n, lane, T0);
    if constexpr (V == 2) {
      const float xs = tile_xscale(tmx);
      mlp_layer_h2q(acc, x2, xvoff, X, 16, lane, xs);
      h2q_unscale(acc, xs, ws2);
    } else if constexpr (X3) {
      mlp_layer_x3q(acc, x2, xvoff, X, 16, lane);
    } else {
      mlp_layer_q<kNTW, kPTW>(acc, ring, w2t, X, 128, lane);
      prime_q<kNTW>(ring, w4t, lane);   // the next tile
    }
    lrelu_bwd_m<kNTW, kPTW>(acc, mk, A.dz[0], tile, n, slope, lane, T0, am ? am + 0 : nullptr);
    // block1.0 point half: d P1[p] += dz1 (the P1 gather's backward).  dz1 goes
    // through LDS so each pair's 1-KB row is added with 4 coalesced 256-B
    // atomic wave instructions (wave w: pairs 16w..16w+15, lane = neuron).
    // d_p1 == NULL: the caller reduces dz1 per point instead (pnr_pairs_to_points).
    __syncthreads();                 // every wave is done reading X (W2^T GEMM)
    if (A.d_p1 == nullptr) continue;
    store_q<kNTW, kPTW>(acc, X, lane, T0);
    __syncthreads();
    for (int i = 0; i < kTP / kPairWaves; ++i) {
      const int col = wid * (kTP / kPairWaves) + i;
      if (tile * kTS + (col >> 3) >= n) break;
      const int32_t pr = A.sv.prow[tile * kTP + col];
      if (pr < 0) continue;
      float* dst = A.d_p1 + (A.pts.used_map ? (int64_t)A.pts.used_map[pr] : (int64_t)pr) * kHid;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nn = lane + 64 * q;
        atomicAdd(dst + nn, X[qaddr(nn, col)]);
      }
    }
    __syncthreads();
  }
  if (am) {   // one global max per workgroup and array
    __syncthreads();
    if (threadIdx.x < 5 && amx[threadIdx.x]) atomicMax(A.sv.dz_absmax + threadIdx.x, amx[threadIdx.x]);
  }
}

// block3.0 extras backward of k_pairs_bwd<true> as its own pass over the pairs:
// g_e = sum_n W3[n, 256 + e] dz3[pair][n] -> d colour (e 0..2) and d dir (e 3..6,
// through R.dir - R.v and <R.dir, R.v>).  One wave per 64 pairs, lane = pair.
__global__ void __launch_bounds__(256) k_extras_bwd(BwdArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t n = eff_n(A.s);
  const int64_t P = n * kKN;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); w * 64 < P; w += waves) {
    const int64_t pair = w * 64 + lane;
    if (pair >= P) continue;
    const int32_t pr = A.sv.prow[pair];
    if (pr < 0) continue;
    float g[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4* z4 = reinterpret_cast<const float4*>(A.dz[2] + pair * kHid);
#pragma unroll 4
    for (int u = 0; u < kHid / 4; ++u) {
      const float4 z = z4[u];
      const float zv[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 7; ++e) g[e] += A.wb.w3e[(4 * u + i) * 7 + e] * zv[i];
    }
    if (A.d_color) {
#pragma unroll
      for (int a = 0; a < 3; ++a) atomicAdd(A.d_color + (int64_t)pr * 3 + a, g[a]);
    }
    if (A.d_dir) {
      float Rw[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) Rw[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
      const int64_t row = sample_row(A.s, pair / kKN);
      const int64_t drow = dir_row(A.s, row);
      const float vd[3] = {A.s.dirs[drow * 3], A.s.dirs[drow * 3 + 1], A.s.dirs[drow * 3 + 2]};
      float vrot[3];
      mat3(Rw, vd, vrot);
      if (A.pts.rw2c) {   // per-point: view dir by the slot-0 matrix, d dir through the pair's
        rot_point(A.pts.rw2c, slot0_point(A.s, row), vd, vrot);
#pragma unroll
        for (int i = 0; i < 9; ++i) Rw[i] = A.pts.rw2c[(int64_t)pr * 9 + i];
      }
      const float gd[3] = {g[3] + vrot[0] * g[6], g[4] + vrot[1] * g[6], g[5] + vrot[2] * g[6]};
#pragma unroll
      for (int i = 0; i < 3; ++i)
        atomicAdd(A.d_dir + (int64_t)pr * 3 + i, Rw[i] * gd[0] + Rw[3 + i] * gd[1] + Rw[6 + i] * gd[2]);
    }
  }
}

// The block3.0 extras per pair without atomics (pnr_aggregate_bwd_extras_rows):
// g_pair[pair] = (g0, g1, g2, g3 + vrot0 g6, g4 + vrot1 g6, g5 + vrot2 g6, 0, 0)
// with g_e = dz3[pair] . W3[:, 256 + e] and vrot the pair's rotated view
// direction; the per-point sums (and the point's Rw^T) follow in
// pnr_pairs_to_points_ex.  Four lanes per pair: a load instruction reads 16 rows'
// 64-B pieces (k_extras_bwd's lane-per-pair loop read 64 rows' 16-B pieces), the
// weights from LDS ([256][8]), two xor steps reduce the four partials.
__global__ void __launch_bounds__(256) k_extras_rows(BwdArgs A, float* __restrict__ g_pair) {
  __shared__ float4 wl[kHid][2];
  for (int i = threadIdx.x; i < kHid; i += blockDim.x) {
    const float* w = A.wb.w3e + i * 7;
    wl[i][0] = make_float4(w[0], w[1], w[2], w[3]);
    wl[i][1] = make_float4(w[4], w[5], w[6], 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane & 3;
  const int64_t n = eff_n(A.s);
  const int64_t P = n * kKN;
  float Ru[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Ru[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
  const int64_t groups = (int64_t)gridDim.x * (blockDim.x >> 2);
  for (int64_t pair = blockIdx.x * (int64_t)(blockDim.x >> 2) + (threadIdx.x >> 2); pair < P; pair += groups) {
    const int32_t pr = A.sv.prow[pair];
    float g[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (pr >= 0) {
      const float4* z4 = reinterpret_cast<const float4*>(A.dz[2] + pair * kHid);
#pragma unroll   // all 16 row pieces in flight (4 at a time: 90 us for 242 MB of dz3)
      for (int j = 0; j < kHid / 16; ++j) {
        const int c4 = 4 * j + q;   // float4 column: neurons 4 c4 .. 4 c4 + 3
        const float4 z = z4[c4];
        const float zv[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 w0 = wl[4 * c4 + i][0], w1 = wl[4 * c4 + i][1];
          g[0] += w0.x * zv[i];
          g[1] += w0.y * zv[i];
          g[2] += w0.z * zv[i];
          g[3] += w0.w * zv[i];
          g[4] += w1.x * zv[i];
          g[5] += w1.y * zv[i];
          g[6] += w1.z * zv[i];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      g[e] += __shfl_xor(g[e], 1);
      g[e] += __shfl_xor(g[e], 2);
    }
    if (q == 0) {
      float vrot[3] = {0.f, 0.f, 0.f};
      if (pr >= 0) {
        const int64_t row = sample_row(A.s, pair / kKN);
        const int64_t drow = dir_row(A.s, row);
        const float vd[3] = {A.s.dirs[drow * 3], A.s.dirs[drow * 3 + 1], A.s.dirs[drow * 3 + 2]};
        mat3(Ru, vd, vrot);
        if (A.pts.rw2c) rot_point(A.pts.rw2c, slot0_point(A.s, row), vd, vrot);
      }
      float4* o = reinterpret_cast<float4*>(g_pair + pair * 8);
      o[0] = make_float4(g[0], g[1], g[2], g[3] + vrot[0] * g[6]);
      o[1] = make_float4(g[4] + vrot[1] * g[6], g[5] + vrot[2] * g[6], 0.f, 0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// d xyz (--xyz_grad 1, neural_points.py:270): the point position enters the
// pair through sampled_xyz (neural_points.py:788-799) -- the world distance
// d = p - s_w, rotated into PE_5's first three channels and giving the inverse-
// distance weight w = 1 / max(|d|, 1e-6), normalised over the K slots
// (point_aggregators.py:775-804) -- and through sampled_xyz_pers =
// w2pers(p) (neural_points.py:635, qpiw.py:102-109), whose deltas
// (x z - x_s z_s, y z - y_s z_s, z - z_s) are PE_5's last three channels.  One
// thread per pair (8 lanes = a sample's K slots, xor8 sums the weight
// normalisation), given d PE_5 = dz1 . W1[:, 224:284] (pnr_gemm_nn) and
// d wt = d alpha a_k + <d hid, h4_k>; atomics into d_xyz.
struct XyzBwdArgs {
  pnr_points pts;
  pnr_samples s;
  pnr_mlp w;
  pnr_agg_saved sv;
  const float* d_feat;   // [n,129]
  const float* d_hid;    // [n,256]
  const float* d_pe;     // [n*8,64] (columns 60..63 unused)
  float* d_xyz;          // [N,3] (+=)
};

__global__ void __launch_bounds__(256) k_xyz_bwd(XyzBwdArgs A) {
  const int64_t n = eff_n(A.s);
  const int64_t pair = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t v = pair >> 3;
  if (v >= n) return;   // whole 8-lane groups
  const int32_t pr = A.sv.prow[pair];
  const bool valid = pr >= 0;
  const int64_t row = sample_row(A.s, v);
  float pw[3] = {0.f, 0.f, 0.f}, d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (valid) pw[a] = A.pts.xyz[(int64_t)pr * 3 + a];
    d[a] = pw[a] - A.s.sample_w[row * 3 + a];
  }
  const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float wl = valid ? 1.f / fmaxf(nrm, 1e-6f) : 0.f;
  const float S = xor8_sum(wl);
  // d wt_k: alpha_s = sum_k wt_k a_k, f_s = sum_k wt_k h4_k
  float dwt = 0.f;
  if (valid && A.sv.vmask[v] != 0) {
    const float pa = A.sv.pa[pair];
    const float a_k = A.w.act_super ? softplus(pa - 1.f) : fmaxf(pa, 0.f);
    const float4* h4 = reinterpret_cast<const float4*>(A.sv.h4 + pair * kHid);
    const float4* dh = reinterpret_cast<const float4*>(A.d_hid + v * kHid);
    float dot = 0.f;
#pragma unroll 8
    for (int q = 0; q < kHid / 4; ++q) {
      const float4 x = h4[q], y = dh[q];
      dot += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    dwt = A.d_feat[v * (kC + 1)] * a_k + dot;
  }
  // wt = wn clamp(conf), wn_k = wl_k / max(S, 1e-8)
  const float confc = (valid && A.pts.conf) ? fminf(fmaxf(A.pts.conf[pr], 1e-4f), 1.f) : 1.f;
  const float dwn = dwt * confc;
  const float dS = S >= 1e-8f ? -xor8_sum(dwn * wl) / (S * S) : 0.f;
  const float dwl = dwn / fmaxf(S, 1e-8f) + dS;
  if (!valid) return;
  float g[3] = {0.f, 0.f, 0.f};
  if (nrm > 1e-6f) {
    const float dn = -dwl / (nrm * nrm * nrm);   // d(1/|d|) / dd = -d / |d|^3
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = dn * d[a];
  }
  // PE_5: value 2(5c + f) = sin(2^f x_c), + 1 = cos(2^f x_c)
  const float* pe = A.sv.pe5 + pair * 64;
  const float* gp = A.d_pe + pair * 64;
  float dd[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const int j = 2 * (5 * c + f);
      acc += (float)(1 << f) * (pe[j + 1] * gp[j] - pe[j] * gp[j + 1]);
    }
    dd[c] = acc;
  }
  // channels 0..2: R.d (d_i gets sum_j R[j][i] dd_j)
  float Rw[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rw[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
  if (A.pts.rw2c) {   // per-point Rw2c: the pair's own matrix
#pragma unroll
    for (int i = 0; i < 9; ++i) Rw[i] = A.pts.rw2c[(int64_t)pr * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] += Rw[i] * dd[0] + Rw[3 + i] * dd[1] + Rw[6 + i] * dd[2];
  // channels 3..5 through the perspective coordinates of the pair's camera
  float c3[3], R[9];
  const int64_t cam = A.s.ray_cam ? (int64_t)A.s.ray_cam[dir_row(A.s, row)] : 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) c3[i] = A.pts.campos[cam * 3 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = A.pts.camrot[cam * 9 + i];
  float xc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    xc[j] = (pw[0] - c3[0]) * R[j] + (pw[1] - c3[1]) * R[3 + j] + (pw[2] - c3[2]) * R[6 + j];
  const float pp[3] = {xc[0] / xc[2], xc[1] / xc[2], xc[2]};
  const float dp0 = dd[3] * pp[2], dp1 = dd[4] * pp[2], dp2 = dd[3] * pp[0] + dd[4] * pp[1] + dd[5];
  const float iz = 1.f / xc[2];
  const float dx0 = dp0 * iz, dx1 = dp1 * iz, dx2 = dp2 - (dp0 * pp[0] + dp1 * pp[1]) * iz;
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] += R[i * 3] * dx0 + R[i * 3 + 1] * dx1 + R[i * 3 + 2] * dx2;
#pragma unroll
  for (int i = 0; i < 3; ++i) atomicAdd(A.d_xyz + (int64_t)pr * 3 + i, g[i]);
}

}  // namespace pnr

using namespace pnr;

template <int V>
static hipError_t pairs_bwd_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pairs_bwd<V>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdLdsBytes);
}

template <int V>
static void launch_pairs_bwd(const BwdArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_pairs_bwd<V>, dim3(grid_for(cdiv(a.s.n_max, kTS), 1, 256 * 2)), dim3(64 * kPairWaves),
                     kBwdLdsBytes, st, a);
}

static int bwd_pairs(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w, const pnr_mlp_bwd* wb,
                     const pnr_mlp_bwd_x3* wbx, const pnr_mlp_bwd_h2* wbh, const pnr_agg_saved* saved,
                     const float* d_feat,
                     const float* d_hid, float* dz1, float* dz2, float* dz3, float* dz4, float* dpa, float* d_p1,
                     float* d_color, float* d_dir, float* d_conf, void* stream) {
  int rc;
  PNR_CHECK_ARG(pts && s && w && wb, "aggregate_bwd: null pointer");
  PNR_CHECK_DEFAULT_DIMS("aggregate_bwd", pts, w);
  if ((rc = check_saved(saved))) return rc;
  PNR_CHECK_ARG((wb->w3e || wbx || wbh) && w->wa && (wbx || wbh || (wb->w4t && wb->w3t && wb->w2t)),
                "aggregate_bwd: null weight");
  PNR_CHECK_ARG(!wbh || (wbh->w4th && wbh->w3th && wbh->w2th && wbh->scale &&
                         (((uintptr_t)wbh->w4th | (uintptr_t)wbh->w3th | (uintptr_t)wbh->w2th) & 15) == 0),
                "aggregate_bwd_h2: null or unaligned split weight pack");
  PNR_CHECK_ARG(!wbx || (wbx->w4tx && wbx->w3tx && wbx->w2tx &&
                         (((uintptr_t)wbx->w4tx | (uintptr_t)wbx->w3tx | (uintptr_t)wbx->w2tx) & 15) == 0),
                "aggregate_bwd_x3: null or unaligned split weight pack");
  PNR_CHECK_ARG(d_feat && d_hid && dz1 && dz2 && dz3 && dz4 && dpa, "aggregate_bwd: null buffer");
  PNR_CHECK_ARG((((uintptr_t)d_hid | (uintptr_t)dz1 | (uintptr_t)dz2 | (uintptr_t)dz3 | (uintptr_t)dz4) & 15) == 0,
                "aggregate_bwd: gradient buffers must be 16-B aligned");
  PNR_CHECK_ARG(s->dirs && s->dir_div >= 1, "aggregate_bwd: sample dirs required");
  PNR_CHECK_ARG(s->K >= 1 && s->K <= kKN, "aggregate_bwd: K=%d unsupported (1..8)", s->K);
  if (s->n_max <= 0) return PNR_OK;
  hipStream_t st = as_stream(stream);
  static bool attr = false;
  if (!attr) {
    PNR_HIP(pairs_bwd_lds<0>());
    PNR_HIP(pairs_bwd_lds<1>());
    PNR_HIP(pairs_bwd_lds<2>());
    attr = true;
  }
  BwdArgs a;
  a.pts = *pts;
  a.s = *s;
  a.w = *w;
  a.wb = *wb;
  a.sv = *saved;
  a.d_feat = d_feat;
  a.d_hid = d_hid;
  a.dz[0] = dz1;
  a.dz[1] = dz2;
  a.dz[2] = dz3;
  a.dz[3] = dz4;
  a.dpa = dpa;
  a.d_p1 = d_p1;
  a.d_color = d_color;
  a.d_dir = d_dir;
  a.d_conf = d_conf;
  a.wx[0] = wbx ? wbx->w4tx : (wbh ? wbh->w4th : nullptr);
  a.wx[1] = wbx ? wbx->w3tx : (wbh ? wbh->w3th : nullptr);
  a.wx[2] = wbx ? wbx->w2tx : (wbh ? wbh->w2th : nullptr);
  a.wxs = wbh ? wbh->scale : nullptr;
  if (wbx || wbh) {
    if (wbh)
      launch_pairs_bwd<2>(a, st);
    else
      launch_pairs_bwd<1>(a, st);
    PNR_LAUNCH_CHECK();
    // wb->w3e == NULL: the caller runs the extras per point inside
    // pnr_pairs_to_points_ex (no float atomics, coalesced dz3 rows)
    if ((d_color || d_dir) && wb->w3e)
      hipLaunchKernelGGL(k_extras_bwd, dim3(grid_for(cdiv(s->n_max * kKN, 64), 4, 2048)), dim3(256), 0, st, a);
  } else
    launch_pairs_bwd<0>(a, st);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_aggregate_bwd_pairs(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                       const pnr_mlp_bwd* wb, const pnr_agg_saved* saved,
                                       const float* d_feat, const float* d_hid, float* dz1, float* dz2,
                                       float* dz3, float* dz4, float* dpa, float* d_p1, float* d_color,
                                       float* d_dir, float* d_conf, void* stream) {
  return bwd_pairs(pts, s, w, wb, nullptr, nullptr, saved, d_feat, d_hid, dz1, dz2, dz3, dz4, dpa, d_p1, d_color,
                   d_dir, d_conf, stream);
}

extern "C" int pnr_aggregate_bwd_pairs_x3(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                          const pnr_mlp_bwd* wb, const pnr_mlp_bwd_x3* wbx,
                                          const pnr_agg_saved* saved, const float* d_feat, const float* d_hid,
                                          float* dz1, float* dz2, float* dz3, float* dz4, float* dpa, float* d_p1,
                                          float* d_color, float* d_dir, float* d_conf, void* stream) {
  PNR_CHECK_ARG(wbx, "aggregate_bwd_x3: null split weight packs");
  return bwd_pairs(pts, s, w, wb, wbx, nullptr, saved, d_feat, d_hid, dz1, dz2, dz3, dz4, dpa, d_p1, d_color, d_dir,
                   d_conf, stream);
}

extern "C" int pnr_aggregate_bwd_pairs_h2(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                          const pnr_mlp_bwd* wb, const pnr_mlp_bwd_h2* wbh,
                                          const pnr_agg_saved* saved, const float* d_feat, const float* d_hid,
                                          float* dz1, float* dz2, float* dz3, float* dz4, float* dpa, float* d_p1,
                                          float* d_color, float* d_dir, float* d_conf, void* stream) {
  PNR_CHECK_ARG(wbh, "aggregate_bwd_h2: null split weight packs");
  return bwd_pairs(pts, s, w, wb, nullptr, wbh, saved, d_feat, d_hid, dz1, dz2, dz3, dz4, dpa, d_p1, d_color, d_dir,
                   d_conf, stream);
}

extern "C" int pnr_aggregate_bwd_xyz(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                     const pnr_agg_saved* saved, const float* d_feat, const float* d_hid,
                                     const float* d_pe, float* d_xyz, void* stream) {
  PNR_CHECK_ARG(pts && s && w && saved && d_feat && d_hid && d_pe && d_xyz, "aggregate_bwd_xyz: null argument");
  PNR_CHECK_DEFAULT_DIMS("aggregate_bwd_xyz", pts, w);
  PNR_CHECK_ARG(pts->xyz && pts->campos && pts->camrot, "aggregate_bwd_xyz: need xyz and the camera tables");
  PNR_CHECK_ARG(saved->prow && saved->pa && saved->h4 && saved->pe5 && saved->vmask,
                "aggregate_bwd_xyz: missing saved activations");
  PNR_CHECK_ARG(s->K <= kKN, "aggregate_bwd_xyz: K > %d", kKN);
  if (s->n_max <= 0) return PNR_OK;
  XyzBwdArgs a;
  a.pts = *pts;
  a.s = *s;
  a.w = *w;
  a.sv = *saved;
  a.d_feat = d_feat;
  a.d_hid = d_hid;
  a.d_pe = d_pe;
  a.d_xyz = d_xyz;
  hipLaunchKernelGGL(k_xyz_bwd, dim3((unsigned)cdiv(s->n_max * kKN, 256)), dim3(256), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_aggregate_bwd_extras_rows(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                             const pnr_agg_saved* saved, const float* w3e, const float* dz3,
                                             float* g_pair, void* stream) {
  PNR_CHECK_ARG(pts && s && w && saved && saved->prow && w3e, "aggregate_bwd_extras_rows: null pointer");
  PNR_CHECK_DEFAULT_DIMS("aggregate_bwd_extras_rows", pts, w);
  PNR_CHECK_ARG(s->n_max == 0 || (dz3 && g_pair && (((uintptr_t)dz3 | (uintptr_t)g_pair) & 15) == 0),
                "aggregate_bwd_extras_rows: dz3 / g_pair must be 16-B aligned");
  PNR_CHECK_ARG(s->dirs && s->dir_div >= 1, "aggregate_bwd_extras_rows: sample dirs required");
  if (s->n_max <= 0) return PNR_OK;
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.pts = *pts;
  a.s = *s;
  a.w = *w;
  a.sv = *saved;
  a.wb.w3e = w3e;
  a.dz[2] = const_cast<float*>(dz3);
  hipLaunchKernelGGL(k_extras_rows, dim3(grid_for(s->n_max * kKN, 64, 4096)), dim3(256), 0, as_stream(stream), a,
                     g_pair);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
