// Fused K-neighbour gather + inverse-distance weights + positional encodings +
// per-(sample, neighbour) MLP + K-weighted sums, then the per-sample colour MLP.
//
// Replaces, for agg_intrp_order 2 / agg_distance_kernel "linear" /
// agg_dist_pers 20 (the lego configuration, dev_scripts/w_n360/lego.sh):
//   NeuralPoints.forward gather             neural_points.py:782-812
//   PointAggregator.forward                 point_aggregators.py:729-816
//     linear kernel + normalisation         point_aggregators.py:421-429, 803-804
//     gradiant_clamp(conf)                  point_aggregators.py:724-726, 810-813
//   viewmlp (order 2)                       point_aggregators.py:488-646
//   positional_encoding                     models/helpers/networks.py:175-190
//
// CDNA4 mapping (three launches):
// k_point_pre: P1[p] = W1[:, :224] . [emb_p, PE_3(emb_p)] + b1 once per point
//   (the point-only half of block1.0; 32 points per wave, 8 accumulator tiles).
// k_pairs: a 4-wave workgroup owns 64 (sample, neighbour) pairs = 8 samples x
//   K=8 and runs the rest of block1 and block3 as Y^T[256 x 64] = W . X^T on
//   v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains; gfx950 has no TF32); wave w
//   owns neuron tiles {2w, 2w+1} for both 32-pair halves, the tile's X^T sits in
//   a quad-row LDS layout (b64 operand reads, b128 activation stores); gather,
//   weights, PE, alpha and the K-sums are fused around the GEMMs.
// k_color: one wave owns 32 valid samples and runs 280->128->128->128 on the
//   same MFMA machinery (4 accumulator tiles).
// Every weight matrix uses one A-operand "fragment" layout
// W_f[t][T][lane] = W[32T + (lane&31)][2t + (lane>>5)] (bias as an extra input
// column), so every weight load is a coalesced 256-B wave load from L2,
// software-pipelined a few k-steps ahead.
#include "agg_quad.h"

namespace pnr {

constexpr int kPitch = 33;         // LDS row pitch (floats) of X^T[k][32 + 1]
constexpr int kXRows = 296;        // >= 286 layer-1 inputs + bias, + x prefetch overrun
constexpr int kWaveLds = kXRows * kPitch;  // floats per wave slice
constexpr size_t kAggLdsBytes = (size_t)4 * kWaveLds * sizeof(float);
constexpr int kPD = 4;             // weight prefetch depth in k-steps of mlp_layer

struct AggArgs {
  pnr_points pts;
  pnr_samples s;
  pnr_mlp w;
  float* p1;                  // [N, 256] per-point block1.0 partial (k_point_pre -> k_pairs)
  float* hid;                 // [n_max, 256] K-summed features (k_pairs -> k_color)
  int32_t* vmask;             // [n_max] sample has >= 1 valid neighbour (k_pairs -> k_color)
  float* out_feat;
  float* out_weight;
  float* out_conf;
  const uint8_t* pair_mask;   // mirror path: validity per (row, k); pidx == NULL
  pnr_agg_saved sv;           // training forward: activations kept for the backward
  const int32_t* run_if = nullptr;   // set: the kernel runs only when *run_if != 0 (the guarded h2 forward's fallback)
};

// The guarded fallback: every workgroup leaves at once unless the h2 range flag is raised.
__device__ __forceinline__ bool skip_run(const AggArgs& A) { return A.run_if && *A.run_if == 0; }

template <int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int T = 0; T < NT; ++T) acc[T] = (f32x16){0.f};
}

// The bias rides in the MFMA: the packed weights carry it as input column
// `kin` (frag_pack), so X^T row kin holds 1 and row kin+1 (if the k-step is
// shared) holds 0.
__device__ __forceinline__ void bias_rows(float* X, int kin, int lane) {
  const int m = lane & 31, h = lane >> 5;
  if ((kin & 1) == 0) X[(kin + h) * kPitch + m] = h ? 0.f : 1.f;
  else if (h == 0) X[kin * kPitch + m] = 1.f;
}

template <int NT>
__device__ __forceinline__ void mfma_step(f32x16 (&acc)[NT], const float (&a)[NT], float x) {
#pragma unroll
  for (int T = 0; T < NT; ++T) acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[T], x, acc[T], 0, 0, 0);
}

// Y^T += W . X^T over nsteps k-steps (2 k-values each); X^T from the wave's
// LDS slice, W in fragment layout, weight loads issued kPD steps ahead.
template <int NT, int NTOT = NT>
__device__ __forceinline__ void mlp_layer(f32x16 (&acc)[NT], const float* __restrict__ wf,
                                          const float* X, int nsteps, int lane) {
  const int m = lane & 31, h = lane >> 5;
  const float* p = wf + lane;
  const float* xr = X + h * kPitch + m;
  float a0[NT], a1[NT], a2[NT], a3[NT];
  load_w<NT, NTOT>(a0, p, 0);
  load_w<NT, NTOT>(a1, p, 1);
  load_w<NT, NTOT>(a2, p, 2);
  load_w<NT, NTOT>(a3, p, 3);
  // B operands of the current 4 k-steps; the next 4 are read from LDS one
  // iteration ahead (rows past the layer's inputs are read but never used)
  float x0 = xr[0], x1 = xr[2 * kPitch], x2 = xr[4 * kPitch], x3 = xr[6 * kPitch];
  int t = 0;
#pragma unroll 1
  for (; t + kPD <= nsteps; t += kPD) {
    const float* xn = xr + 2 * (t + kPD) * kPitch;
    // sched_barrier(0) pins the software pipeline: hipcc otherwise sinks the
    // next iteration's LDS reads next to their use (exposed LDS latency)
    mfma_step<NT>(acc, a0, x0);
    const float y0 = xn[0], y1 = xn[2 * kPitch], y2 = xn[4 * kPitch], y3 = xn[6 * kPitch];
    load_w<NT, NTOT>(a0, p, t + 4);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<NT>(acc, a1, x1);
    load_w<NT, NTOT>(a1, p, t + 5);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<NT>(acc, a2, x2);
    load_w<NT, NTOT>(a2, p, t + 6);
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<NT>(acc, a3, x3);
    load_w<NT, NTOT>(a3, p, t + 7);
    __builtin_amdgcn_sched_barrier(0);
    x0 = y0;
    x1 = y1;
    x2 = y2;
    x3 = y3;
  }
  const int rem = nsteps - t;  // 0..3
  if (rem > 0) mfma_step<NT>(acc, a0, x0);
  if (rem > 1) mfma_step<NT>(acc, a1, x1);
  if (rem > 2) mfma_step<NT>(acc, a2, x2);
}

// Activated accumulator -> X^T rows in natural neuron order.
template <int NT>
__device__ __forceinline__ void store_act(const f32x16 (&acc)[NT], float* X, float s, int lane, int T0 = 0) {
  const int m = lane & 31, h = lane >> 5;
#pragma unroll
  for (int T = 0; T < NT; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) X[(32 * (T0 + T) + acc_row(r, h)) * kPitch + m] = lrelu(acc[T][r], s);
}

// Per-point half of block1.0 (exact split of the 284-input Linear): the
// embedding and its 3-band PE depend only on the point, so
// P1[p] = W1[:, :224] . [emb_p, PE_3(emb_p)] + b1 is evaluated once per point
// and gathered per pair instead of being recomputed for every (sample,
// neighbour) pair that references the point (~22x reuse at 2 M points).
__global__ void __launch_bounds__(kAggBlock, 1) k_point_pre(AggArgs A) {
  if (skip_run(A)) return;
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* X = lds_dyn + wid * kWaveLds;
  const int m = lane & 31, h = lane >> 5;
  const int64_t np = p1_rows(A.pts);   // P1 rows
  const int64_t ntiles = cdiv(np, 32);
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wid; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t pt = tile * 32 + m;                         // P1 row
    const bool act = pt < np;
    const int64_t prow = act ? (A.pts.used ? (int64_t)A.pts.used[pt] : pt) : 0;   // point row
    // lane half h owns embedding channels [16h, 16h+16): the channel itself (row c)
    // and its 3-band PE (rows 32 + 2(3c+f) + {0: sin, 1: cos}); angle doubling
    // from one sincos: sin 2x = 2 sin x cos x, cos 2x = (c - s)(c + s).
    const float* e = A.pts.emb + prow * kEmb + 16 * h;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      float4 e4 = act ? reinterpret_cast<const float4*>(e)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = 16 * h + 4 * q + u;
        X[c * kPitch + m] = ev[u];
        float s0, c0;
        sincosf(ev[u], &s0, &c0);
        const float s1 = 2.f * s0 * c0, c1 = (c0 - s0) * (c0 + s0);
        const float s2 = 2.f * s1 * c1, c2 = (c1 - s1) * (c1 + s1);
        const int r0 = kEmb + 6 * c;
        X[(r0 + 0) * kPitch + m] = s0;
        X[(r0 + 1) * kPitch + m] = c0;
        X[(r0 + 2) * kPitch + m] = s1;
        X[(r0 + 3) * kPitch + m] = c1;
        X[(r0 + 4) * kPitch + m] = s2;
        X[(r0 + 5) * kPitch + m] = c2;
      }
    }
    bias_rows(X, kEmb * 7, lane);   // row 224 = 1 (bias column), 225 = 0
    wave_sync();
    f32x16 acc[8];
    zero_acc<8>(acc);
    mlp_layer<8>(acc, A.w.w1af, X, 113, lane);
    if (act) {
      float4* o = reinterpret_cast<float4*>(A.p1 + pt * kHid);
#pragma unroll
      for (int T = 0; T < 8; ++T)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[8 * T + 2 * q + h] = make_float4(acc[T][4 * q], acc[T][4 * q + 1], acc[T][4 * q + 2], acc[T][4 * q + 3]);
    }
    wave_sync();
  }
}

// Post-activation accumulator tiles -> [row][ld] global rows (training saves);
// lane column m = row offset, rows of tile T at columns 32T + 8q + 4h.
template <int NT>
__device__ __forceinline__ void save_rows(const f32x16 (&acc)[NT], float* dst, int64_t row, int ld, float s,
                                          int lane, int T0 = 0) {
  const int h = lane >> 5;
#pragma unroll
  for (int T = 0; T < NT; ++T)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(dst + row * ld + 32 * (T0 + T) + 8 * q + 4 * h) =
          make_float4(lrelu(acc[T][4 * q], s), lrelu(acc[T][4 * q + 1], s), lrelu(acc[T][4 * q + 2], s),
                      lrelu(acc[T][4 * q + 3], s));
}



// ---------------------------------------------------------------------------
// k_pairs: one workgroup (4 waves) owns a tile of 64 pairs = 8 samples x K=8.
// Wave w computes neuron tiles {2w, 2w+1} for both 32-pair halves of the tile
// (4 accumulator tiles, 64 VGPRs), so every 256-B weight fragment fetched
// from L2 feeds two MFMAs and every LDS B-operand read feeds two.  Two
// workgroups per CU (2 waves per SIMD) overlap one tile's gather / PE / tail
// with the other's MFMA stream.  The tile's layer input X^T sits in quad rows
// (agg_quad.h).
constexpr int kQRows = (264 + 2 * kQD + 3) / 4;  // layer-3 input rows + x prefetch overrun
constexpr int kPairsLdsFloats = kQRows * kQP + kTP /*wt*/ + 4 * kTP /*alpha parts*/ + kTS /*flags*/ +
                                8 * kTP /*block3 extras*/;
static_assert(kQD <= kPackPad && kPD <= kPackPad, "prefetch deeper than the packed padding");
constexpr size_t kPairsLdsBytes = (size_t)kPairsLdsFloats * sizeof(float);

// Activated accumulators -> quad rows (one b128 per accumulator quad).
template <int NT, int PT>
__device__ __forceinline__ void store_act_q(const f32x16 (&acc)[PT * NT], float* X, float s, int lane,
                                            int T0) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x16& v = acc[pt * NT + T];
        *reinterpret_cast<float4*>(X + (8 * (T0 + T) + 2 * q + h) * kQP + 4 * (32 * pt + c)) =
            make_float4(lrelu(v[4 * q], s), lrelu(v[4 * q + 2], s), lrelu(v[4 * q + 1], s),
                        lrelu(v[4 * q + 3], s));
      }
}

// X^T row kin = 1 (bias column of the packed weights), row kin + 1 = 0 when
// the k-step is shared; one wave, lane = pair column.
__device__ __forceinline__ void bias_rows_q(float* X, int kin, int lane) {
  X[qaddr(kin, lane)] = 1.f;
  if ((kin & 1) == 0) X[qaddr(kin + 1, lane)] = 0.f;
}


// Training save of a colour-branch tile (output tile T0, PT sample halves) -> dst[v][128].
template <int PT>
__device__ __forceinline__ void save_cols(const f32x16 (&acc)[PT], float* dst, int64_t v0, int64_t n, float s,
                                          int lane, int T0) {
  const int c = lane & 31;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int64_t v = v0 + 32 * pt + c;
    if (v >= n) continue;
    f32x16 one[1] = {acc[pt]};
    save_rows<1>(one, dst, v, kC, s, lane, T0);
  }
}

// Training save of a tile's post-activation quad (both halves) -> dst[pair][256].
// Also keeps the LeakyReLU derivative as bits: mask[pair][16 * layer + 2T + h]
// bit r = (pre-activation of accumulator register r of tile T, lane half h > 0).
template <int NT, int PT>
__device__ __forceinline__ void save_pairs_q(const f32x16 (&acc)[PT * NT], float* dst, uint16_t* mask,
                                             int layer, int64_t tile, int64_t n, float s, int lane, int T0) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int col = 32 * pt + c;
    if (tile * kTS + (col >> 3) >= n) continue;
    f32x16 one[NT];
#pragma unroll
    for (int T = 0; T < NT; ++T) one[T] = acc[pt * NT + T];
    save_rows<NT>(one, dst, tile * kTP + col, kHid, s, lane, T0);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      unsigned bits = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) bits |= (one[T][r] > 0.f ? 1u : 0u) << r;
      mask[(tile * kTP + col) * 64 + 16 * layer + 2 * (T0 + T) + h] = (uint16_t)bits;
    }
  }
}

constexpr int kPairSub = 1;   // tiles per workgroup sharing barriers (and weight-fragment fetches)

template <bool TRAIN>
__global__ void __launch_bounds__(64 * kPairWaves * kPairSub, 2 / kPairSub) k_pairs(AggArgs A) {
  if (skip_run(A)) return;
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  const int sub = (threadIdx.x >> 6) / kPairWaves;   // which of the workgroup's tiles
  float* X = lds_dyn + sub * kPairsLdsFloats;  // quad rows [kQRows][kQP]
  float* wtL = X + kQRows * kQP;               // [64] per-pair blend weight w_k * conf_k
  float* apart = wtL + kTP;                    // [4][64] alpha partial dots
  int* sflag = reinterpret_cast<int*>(apart + 4 * kTP);  // [8] sample has a valid neighbour
  float* exL = apart + 4 * kTP + kTS;          // [8][64] block3.0 extra inputs, parked from the gather
  const int lane = threadIdx.x & 63, wid = (threadIdx.x >> 6) % kPairWaves;
  const int c = lane & 31, h = lane >> 5;
  const int j = lane >> 3, k = lane & 7;       // gather layout: lane = pair column
  const int T0 = wid * kNTW;
  const int K = A.s.K;
  const int64_t n = eff_n(A.s);
  const int64_t ntiles = cdiv(n, kTS);
  const int64_t ngroups = cdiv(ntiles, kPairSub);
  const float neg = A.w.neg_slope;
  float Rw[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rw[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
  float cam_c[3] = {0.f, 0.f, 0.f}, cam_R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (!A.pts.pers) {
#pragma unroll
    for (int i = 0; i < 3; ++i) cam_c[i] = A.pts.campos[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) cam_R[i] = A.pts.camrot[i];
  }
  const float* w1b = A.w.w1bf + T0 * 64;
  const float* w2 = A.w.w2f + T0 * 64;
  const float* w3 = A.w.w3f + T0 * 64;
  const float* w4 = A.w.w4f + T0 * 64;
  float ring[kQD][kNTW];
  prime_q<kNTW>(ring, w1b, lane);

  for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int64_t tile = grp * kPairSub + sub;   // past ntiles: every pair inactive
    // ------------------------------------------------------------ gather (neural_points.py:788-799)
    const int64_t v = tile * kTS + j;
    const bool active = v < n;
    const int64_t row = active ? sample_row(A.s, v) : 0;
    int64_t prow = -1;  // point row
    bool valid = false;
    if (active && k < K) {
      if (A.s.pidx) {
        const int pid = A.s.pidx[row * K + k];
        valid = pid >= 0;
        prow = valid ? pid : 0;  // torch.clamp(sample_pidx, min=0)
      } else {
        prow = row * K + k;
        valid = A.pair_mask[prow] != 0;
      }
    }
    // this wave's neuron tiles of the gathered per-point block1.0 partial P1
    // (bias included) for the pairs of both halves (MFMA layout: column c)
    f32x16 acc[kPTW * kNTW];
#pragma unroll
    for (int pt = 0; pt < kPTW; ++pt) {
      const int64_t pr_pt = __shfl(prow, 32 * pt + c);
      const bool v_pt = __shfl((int)valid, 32 * pt + c) != 0;
      if (v_pt) {
        const int64_t p1r = A.pts.used_map ? (int64_t)A.pts.used_map[pr_pt] : pr_pt;
        const float4* pr = reinterpret_cast<const float4*>(A.p1 + p1r * kHid);
#pragma unroll
        for (int T = 0; T < kNTW; ++T)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 v4 = pr[8 * (T0 + T) + 2 * q + h];
            acc[pt * kNTW + T][4 * q] = v4.x;
            acc[pt * kNTW + T][4 * q + 1] = v4.y;
            acc[pt * kNTW + T][4 * q + 2] = v4.z;
            acc[pt * kNTW + T][4 * q + 3] = v4.w;
          }
      } else {
#pragma unroll
        for (int T = 0; T < kNTW; ++T) acc[pt * kNTW + T] = (f32x16){0.f};
      }
    }
    float sw[3] = {0.f, 0.f, 0.f}, sp[3] = {0.f, 0.f, 0.f}, vd[3] = {0.f, 0.f, 0.f};
    int64_t drow = 0;
    if (active) {
      drow = dir_row(A.s, row);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sw[a] = A.s.sample_w[row * 3 + a];
        sp[a] = A.s.sample_p[row * 3 + a];
        vd[a] = A.s.dirs[drow * 3 + a];
      }
    }
    float pw[3] = {0.f, 0.f, 0.f}, pp[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f},
          pdir[3] = {0.f, 0.f, 0.f};
    float cf = 1.f;
    if (valid) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        pw[a] = A.pts.xyz[prow * 3 + a];
        col[a] = A.pts.color ? A.pts.color[prow * 3 + a] : 0.f;
        pdir[a] = A.pts.dir ? A.pts.dir[prow * 3 + a] : 0.f;
      }
      if (A.pts.pers) {
#pragma unroll
        for (int a = 0; a < 3; ++a) pp[a] = A.pts.pers[prow * 3 + a];
      } else {
        pair_pers(A.pts, A.s, drow, pw, cam_c, cam_R, pp);
      }
    }
    if (A.pts.conf && prow >= 0) cf = A.pts.conf[prow];
    // dists, agg_dist_pers == 20 (point_aggregators.py:775-783)
    float d6[6];
    d6[0] = pw[0] - sw[0];
    d6[1] = pw[1] - sw[1];
    d6[2] = pw[2] - sw[2];
    d6[3] = pp[0] * pp[2] - sp[0] * sp[2];
    d6[4] = pp[1] * pp[2] - sp[1] * sp[2];
    d6[5] = pp[2] - sp[2];
    // linear kernel (point_aggregators.py:421-429) and normalisation (:803-804)
    const float nrm = sqrtf(d6[0] * d6[0] + d6[1] * d6[1] + d6[2] * d6[2]);
    const float wl = valid ? 1.f / fmaxf(nrm, 1e-6f) : 0.f;
    const float wsum = xor8_sum(wl);
    const float wn = wl / fmaxf(wsum, 1e-8f);
    const float confc = fminf(fmaxf(cf, 1e-4f), 1.f);
    const float wt = wn * confc;
    const bool samp_valid = xor8_sum(valid ? 1.f : 0.f) > 0.f;
    // rotated distance / direction inputs (point_aggregators.py:506, 526, 566-570)
    float dr6[6];
    mat3(Rw, d6, dr6);
    dr6[3] = d6[3];
    dr6[4] = d6[4];
    dr6[5] = d6[5];
    float vrot[3], drot[3];
    mat3(Rw, vd, vrot);
    mat3(Rw, pdir, drot);
    if (A.pts.rw2c) {   // per-point Rw2c (agg_common.h rot_point)
      rot_point(A.pts.rw2c, prow, d6, dr6);
      rot_point(A.pts.rw2c, prow, pdir, drot);
      rot_point(A.pts.rw2c, active ? slot0_point(A.s, row) : 0, vd, vrot);
    }
    if (wid == 0) {
      // block3 inputs 256..263: colour(3), R.dir - R.v (3), <R.dir, R.v> (1), bias 1
      const float dot = drot[0] * vrot[0] + drot[1] * vrot[1] + drot[2] * vrot[2];
      const float ex[8] = {col[0], col[1], col[2], drot[0] - vrot[0],
                           drot[1] - vrot[1], drot[2] - vrot[2], dot, 1.f};
#pragma unroll
      for (int e = 0; e < 8; ++e) exL[e * kTP + lane] = ex[e];
      if (TRAIN && active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) A.sv.x3e[(tile * kTP + lane) * 32 + e] = ex[e];
        float4* z = reinterpret_cast<float4*>(A.sv.x3e + (tile * kTP + lane) * 32 + 8);
#pragma unroll
        for (int e = 0; e < 6; ++e) z[e] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (active && k < K) {
        if (A.out_weight) A.out_weight[row * K + k] = wn;
        if (A.out_conf) A.out_conf[row * K + k] = confc;
      }
      wtL[lane] = wt;
      if (k == 0) sflag[j] = active && samp_valid;
      if (TRAIN && active) {
        const int64_t pr = tile * kTP + lane;
        A.sv.wt[pr] = wt;
        A.sv.wn[pr] = wn;
        A.sv.prow[pr] = valid ? (int32_t)prow : -1;
      }
    }
    // 5-band PE of the 6-d rotated distance -> rows 2e + {0: sin, 1: cos},
    // e = 5 ch + f (block1.0 columns 224..283); wave w owns e = w (mod 4)
    {
#pragma unroll 1
      for (int e = wid; e < 30; e += kPairWaves) {
        const int ch = e / 5, f = e - 5 * ch;
        float dc = dr6[0];
        dc = ch == 1 ? dr6[1] : dc;
        dc = ch == 2 ? dr6[2] : dc;
        dc = ch == 3 ? dr6[3] : dc;
        dc = ch == 4 ? dr6[4] : dc;
        dc = ch == 5 ? dr6[5] : dc;
        float sn, cs;
        sincosf(dc * (float)(1 << f), &sn, &cs);
        X[qaddr(2 * e, lane)] = sn;
        X[qaddr(2 * e + 1, lane)] = cs;
        if (TRAIN && active) {
          float* pe = A.sv.pe5 + (tile * kTP + lane) * 64 + 2 * e;
          pe[0] = sn;
          pe[1] = cs;
        }
      }
    }
    if (TRAIN && active && wid == kPairWaves - 1)   // pe5 rows are padded to 64 for the dW GEMM
      *reinterpret_cast<float4*>(A.sv.pe5 + (tile * kTP + lane) * 64 + 60) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    // ------------------------------------------------------------ block1: 284 -> 256 -> 256
    mlp_layer_q<kNTW, kPTW>(acc, ring, w1b, X, 30, lane);   // + W1[:, 224:284] . PE_5(dist)
    prime_q<kNTW>(ring, w2, lane);
    __syncthreads();
    store_act_q<kNTW, kPTW>(acc, X, neg, lane, T0);
    if (TRAIN) save_pairs_q<kNTW, kPTW>(acc, A.sv.h1, A.sv.mask, 0, tile, n, neg, lane, T0);
    if (wid == 0) bias_rows_q(X, 256, lane);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    mlp_layer_q<kNTW, kPTW>(acc, ring, w2, X, 129, lane);
    prime_q<kNTW>(ring, w3, lane);
    __syncthreads();
    store_act_q<kNTW, kPTW>(acc, X, neg, lane, T0);
    if (TRAIN) save_pairs_q<kNTW, kPTW>(acc, A.sv.h2, A.sv.mask, 1, tile, n, neg, lane, T0);
    // block3 inputs rows 256..263 (parked in exL by the gather)
    if (wid == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) X[qaddr(256 + e, lane)] = exL[e * kTP + lane];
    }
    __syncthreads();
    // ------------------------------------------------------------ block3: 263 -> 256 -> 256
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    mlp_layer_q<kNTW, kPTW>(acc, ring, w3, X, 132, lane);
    prime_q<kNTW>(ring, w4, lane);
    __syncthreads();
    store_act_q<kNTW, kPTW>(acc, X, neg, lane, T0);
    if (TRAIN) save_pairs_q<kNTW, kPTW>(acc, A.sv.h3, A.sv.mask, 2, tile, n, neg, lane, T0);
    if (wid == 0) bias_rows_q(X, 256, lane);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPTW * kNTW; ++i) acc[i] = (f32x16){0.f};
    mlp_layer_q<kNTW, kPTW>(acc, ring, w4, X, 129, lane);
    prime_q<kNTW>(ring, w1b, lane);                   // the next tile's layer 1
    if (TRAIN) save_pairs_q<kNTW, kPTW>(acc, A.sv.h4, A.sv.mask, 3, tile, n, neg, lane, T0);
    {
      // ---------------------------------------------------------- alpha + K sums from registers
      // h4 = lrelu(acc) never goes to LDS.  alpha: each lane dots its 32 rows of
      // the wave's 64 neurons with W_a, the two lane halves and the 4 waves are
      // summed through LDS.  K sums (point_aggregators.py:622-628): the 8 pairs
      // of a sample are 8 adjacent lanes; a 3-round DPP reduce-scatter (row
      // half-mirror, quad xor 2, quad xor 1) leaves lane i of the 8 with the
      // sums of accumulator registers 2i, 2i+1 = two adjacent neurons.
      float pa_part[kPTW] = {0.f, 0.f};
#pragma unroll
      for (int pt = 0; pt < kPTW; ++pt) {
        const float wtp = wtL[32 * pt + c];
        const int sj = (32 * pt + c) >> 3;
        const int64_t vo = tile * kTS + sj;
        const bool wr = vo < n && sflag[sj];
        const int i8 = c & 7;
#pragma unroll
        for (int T = 0; T < kNTW; ++T) {
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float hv = lrelu(acc[pt * kNTW + T][r], neg);
            pa_part[pt] += A.w.wa[32 * (T0 + T) + acc_row(r, h)] * hv;
            v[r] = wtp * hv;
          }
          float w8[8], w4[4], w2[2];
          const bool b2 = (i8 & 4) != 0, b1 = (i8 & 2) != 0, b0 = (i8 & 1) != 0;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float send = b2 ? v[q] : v[q + 8];
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send),
                                                                                  0x141, 0xf, 0xf, false));
            w8[q] = (b2 ? v[q + 8] : v[q]) + recv;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float send = b1 ? w8[q] : w8[q + 4];
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send),
                                                                                  0x4E, 0xf, 0xf, false));
            w4[q] = (b1 ? w8[q + 4] : w8[q]) + recv;
          }
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float send = b0 ? w4[q] : w4[q + 2];
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send),
                                                                                  0xB1, 0xf, 0xf, false));
            w2[q] = (b0 ? w4[q + 2] : w4[q]) + recv;
          }
          // registers 2 i8, 2 i8 + 1 -> rows (2 i8 & 3) + 8 (i8 >> 1) + 4h (+1)
          if (wr)
            *reinterpret_cast<float2*>(A.hid + vo * kHid + 32 * (T0 + T) + ((2 * i8) & 3) + 8 * (i8 >> 1) + 4 * h) =
                make_float2(w2[0], w2[1]);
        }
        pa_part[pt] += __shfl_xor(pa_part[pt], 32);
      }
      if (h == 0) {
        apart[wid * kTP + c] = pa_part[0];
        apart[wid * kTP + 32 + c] = pa_part[1];
      }
      __syncthreads();
      if (wid == 0) {
        const float pa = apart[lane] + apart[kTP + lane] + apart[2 * kTP + lane] + apart[3 * kTP + lane] +
                         A.w.ba[0];
        const float alpha_k = A.w.act_super ? softplus(pa - 1.f) : fmaxf(pa, 0.f);
        const float alpha_s = xor8_sum(wtL[lane] * alpha_k);   // point_aggregators.py:608-614
        const int64_t vo = tile * kTS + j;
        if (TRAIN && vo < n) A.sv.pa[tile * kTP + lane] = pa;
        if (k == 0 && vo < n) {
          A.vmask[vo] = sflag[j];
          if (sflag[j]) A.out_feat[vo * (kC + 1)] = alpha_s;
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// k_color: the colour branch 280 -> 128 -> 128 -> 128 (LeakyReLU each,
// point_aggregators.py:630-638) for 64 valid samples per 4-wave workgroup, on
// the same quad-row LDS pipeline as k_pairs: wave w owns output tile w for
// both 32-sample halves (2 MFMAs per weight fragment).  Input rows: the
// K-summed features hid (transposed from [sample][256] rows with one float4
// per lane), the 4-band view-direction PE (sin block, cos block, :506-512)
// and the bias row.
constexpr int kColWaves = 4;
constexpr int kColQRows = (282 + 2 * kQD + 3) / 4;
constexpr size_t kColLdsBytes = (size_t)kColQRows * kQP * sizeof(float);

template <bool TRAIN>
__global__ void __launch_bounds__(64 * kColWaves, 2) k_color(AggArgs A) {
  if (skip_run(A)) return;
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  float* X = lds_dyn;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int64_t n = eff_n(A.s);
  const int64_t ntiles = cdiv(n, kTP);
  const float neg = A.w.neg_slope;
  float Rw[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rw[i] = A.w.rw2c ? A.w.rw2c[i] : (i % 4 == 0 ? 1.f : 0.f);
  const float* w1 = A.w.wc1f + wid * 64;
  const float* w2 = A.w.wc2f + wid * 64;
  const float* w3 = A.w.wc3f + wid * 64;
  float ring[kQD][1];
  prime_q<1, 4>(ring, w1, lane);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t v0 = tile * kTP;
    // hid rows -> X^T rows 0..255 (wave w: samples 16w..16w+15, lane = neuron quad)
    for (int i = 0; i < kTP / kColWaves; ++i) {
      const int col = wid * (kTP / kColWaves) + i;
      const int64_t v = v0 + col;
      const bool ok = v < n && A.vmask[v] != 0;
      const float4 f4 = ok ? reinterpret_cast<const float4*>(A.hid + v * kHid)[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(X + lane * kQP + 4 * col) = make_float4(f4.x, f4.z, f4.y, f4.w);
    }
    // view-direction PE (ori dropped): rows 256 + 4ch + f = sin, 268 + 4ch + f = cos;
    // wave ch < 3 owns channel ch, wave 3 the bias rows 280 (1) / 281 (0); lane = sample
    {
      const int64_t v = v0 + lane;
      if (wid < 3) {
        float vrot[3] = {0.f, 0.f, 0.f};
        if (v < n) {
          const int64_t row = sample_row(A.s, v);
          const int64_t drow = dir_row(A.s, row);
          const float vd[3] = {A.s.dirs[drow * 3], A.s.dirs[drow * 3 + 1], A.s.dirs[drow * 3 + 2]};
          mat3(Rw, vd, vrot);
          if (A.pts.rw2c) rot_point(A.pts.rw2c, slot0_point(A.s, row), vd, vrot);
        }
        const float x = wid == 0 ? vrot[0] : (wid == 1 ? vrot[1] : vrot[2]);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          float sn, cs;
          sincosf(x * (float)(1 << f), &sn, &cs);
          X[qaddr(kHid + 4 * wid + f, lane)] = sn;
          X[qaddr(kHid + 12 + 4 * wid + f, lane)] = cs;
          if (TRAIN && v < n) {
            A.sv.vpe[v * 24 + 4 * wid + f] = sn;
            A.sv.vpe[v * 24 + 12 + 4 * wid + f] = cs;
          }
        }
      } else {
        X[qaddr(kCin, lane)] = 1.f;
        X[qaddr(kCin + 1, lane)] = 0.f;
      }
    }
    __syncthreads();
    f32x16 acc[2];
    acc[0] = acc[1] = (f32x16){0.f};
    mlp_layer_q<1, 2, 4>(acc, ring, w1, X, 141, lane);   // 280 inputs + bias column
    prime_q<1, 4>(ring, w2, lane);
    __syncthreads();
    store_act_q<1, 2>(acc, X, neg, lane, wid);
    if (wid == 0) bias_rows_q(X, kC, lane);
    if (TRAIN) save_cols<2>(acc, A.sv.hc1, v0, n, neg, lane, wid);
    __syncthreads();
    acc[0] = acc[1] = (f32x16){0.f};
    mlp_layer_q<1, 2, 4>(acc, ring, w2, X, 65, lane);
    prime_q<1, 4>(ring, w3, lane);
    __syncthreads();
    store_act_q<1, 2>(acc, X, neg, lane, wid);
    if (wid == 0) bias_rows_q(X, kC, lane);
    if (TRAIN) save_cols<2>(acc, A.sv.hc2, v0, n, neg, lane, wid);
    __syncthreads();
    acc[0] = acc[1] = (f32x16){0.f};
    mlp_layer_q<1, 2, 4>(acc, ring, w3, X, 65, lane);
    prime_q<1, 4>(ring, w1, lane);   // the next tile
    if (TRAIN) save_cols<2>(acc, A.sv.hc3, v0, n, neg, lane, wid);
    // out_feat[v, 1 + n] (valid samples only; the others keep their zeros)
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      const int64_t v = v0 + 32 * pt + c;
      if (v >= n || A.vmask[v] == 0) continue;
      float* o = A.out_feat + v * (kC + 1) + 1 + 32 * wid + 4 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[8 * q + i] = lrelu(acc[pt][4 * q + i], neg);
    }
    __syncthreads();
  }
}

constexpr int kStagePre = 1, kStagePairs = 2, kStageColor = 4, kStageAll = 7;

template <bool TRAIN>
int launch_t(const AggArgs& a, hipStream_t st, int stages = kStageAll) {
  static bool attr = false;
  if (!attr) {
    PNR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pairs<TRAIN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPairsLdsBytes * kPairSub)));
    PNR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_point_pre),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAggLdsBytes));
    PNR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_color<TRAIN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kColLdsBytes));
    attr = true;
  }
  if ((stages & kStagePre) && !a.pts.p1_ready) {
    hipLaunchKernelGGL(k_point_pre, dim3(grid_for(cdiv(a.pts.used ? a.pts.n_used : a.pts.n, 32), 4, 256)),
                       dim3(kAggBlock), kAggLdsBytes, st, a);
    PNR_LAUNCH_CHECK();
  }
  if (stages & kStagePairs) {
    const int64_t tiles = cdiv(a.s.n_max, kTS);
    hipLaunchKernelGGL(k_pairs<TRAIN>, dim3(grid_for(cdiv(tiles, kPairSub), 1, 256 * 2 / kPairSub)),
                       dim3(64 * kPairWaves * kPairSub), kPairsLdsBytes * kPairSub, st, a);
    PNR_LAUNCH_CHECK();
  }
  if (stages & kStageColor) {
    const int64_t ctiles = cdiv(a.s.n_max, kTP);
    hipLaunchKernelGGL(k_color<TRAIN>, dim3(grid_for(ctiles, 1, 256 * 2)), dim3(64 * kColWaves), kColLdsBytes, st,
                       a);
    PNR_LAUNCH_CHECK();
  }
  return PNR_OK;
}

// hid rows for n_max samples rounded up to whole 64-sample tiles (the h2
// planes layout, kHidTile in aggregate_x3.hip)
static int64_t hid_rows(int64_t n_max) { return cdiv(n_max > 0 ? n_max : 1, 64) * 64; }

static size_t scratch_need(int64_t n_max, int64_t n_points) {
  const int64_t nm = hid_rows(n_max);
  // + 8 ints: the split kernels' tile counters (k_pairs_x3 / k_pairs_h2, one per XCD group), padded to 16 B
  return ((size_t)nm * kHid + (size_t)cdiv(nm, 4) * 4 + 16 + (size_t)(n_points > 0 ? n_points : 1) * kHid) *
         sizeof(float);
}

// scratch = P1 [n_p1, 256] | hid [n_max, 256] | vmask | tile counter: P1 first,
// so its place does not depend on n_max and a later call may reuse it
// (pnr_points.p1_ready).  Returns the split kernels' tile counter, which stays
// in the scratch when a training call redirects hid / vmask to the saved arrays.
// With a P1 table of the caller's (p1_table) the scratch keeps the layout of
// n_p1 = 0 (one unused row), so P1 outlives the scratch.
static int32_t* carve(AggArgs& a, void* scratch, int64_t n_max, int64_t n_p1, float* p1_table) {
  const int64_t nm = hid_rows(n_max);
  if (p1_table) n_p1 = 0;
  a.p1 = p1_table ? p1_table : static_cast<float*>(scratch);
  a.hid = static_cast<float*>(scratch) + (n_p1 > 0 ? n_p1 : 1) * kHid;
  a.vmask = reinterpret_cast<int32_t*>(a.hid + nm * kHid);
  return a.vmask + cdiv(nm, 4) * 4;
}

static int check_common(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w, float* out_feat,
                        void* scratch, size_t scratch_bytes, const float* p1_table) {
  PNR_CHECK_ARG(pts && s && w && out_feat, "aggregate: null pointer");
  PNR_CHECK_ARG(pts->xyz && pts->emb, "aggregate: point xyz/emb required");
  PNR_CHECK_ARG(s->sample_w && s->sample_p && s->dirs, "aggregate: sample arrays required");
  PNR_CHECK_ARG(s->K >= 1 && s->K <= kKN, "aggregate: K=%d unsupported (1..8)", s->K);
  PNR_CHECK_ARG(s->dir_div >= 1, "aggregate: dir_div must be >= 1");
  PNR_CHECK_ARG(w->w1af && w->w1bf && w->w2f && w->b2 && w->w3f && w->b3 && w->w4f && w->b4 && w->wa &&
                    w->ba && w->wc1f && w->bc1 && w->wc2f && w->bc2 && w->wc3f && w->bc3,
                "aggregate: null weight");
  PNR_CHECK_ARG(pts->emb_dim >= 0 && pts->emb_dim <= 64, "aggregate: emb_dim %d unsupported (1..64, 0 = 32)",
                pts->emb_dim);
  PNR_CHECK_ARG(w->intrp_order >= 0 && w->intrp_order <= 2, "aggregate: intrp_order %d unsupported (0, 1, 2)",
                w->intrp_order);
  // the wide per-point kernels read emb with dword loads; the 32-wide ones with b128
  PNR_CHECK_ARG(((uintptr_t)pts->emb & (emb_width(*pts) == kEmb ? 15 : 3)) == 0,
                "aggregate: emb must be 16-B aligned (4-B with emb_dim != 32)");
  PNR_CHECK_ARG(scratch && ((uintptr_t)scratch & 15) == 0, "aggregate: 16-B aligned scratch required");
  PNR_CHECK_ARG(pts->n > 0, "aggregate: empty point table");
  PNR_CHECK_ARG(!pts->used || (pts->used_map && pts->n_used >= 0 && pts->n_used <= pts->n),
                "aggregate: used list needs used_map and 0 <= n_used <= n");
  PNR_CHECK_ARG(((uintptr_t)p1_table & 15) == 0, "aggregate: p1_table must be 16-B aligned");
  PNR_CHECK_ARG(scratch_bytes >= scratch_need(s->n_max, p1_table ? 0 : pts->used ? pts->n_used : pts->n),
                "aggregate: scratch too small (%zu bytes for %lld samples, %lld points)", scratch_bytes,
                (long long)s->n_max, (long long)pts->n);
  return PNR_OK;
}

int check_saved(const pnr_agg_saved* sv) {
  PNR_CHECK_ARG(sv, "aggregate train: null saved struct");
  PNR_CHECK_ARG(sv->h1 && sv->h2 && sv->h3 && sv->h4 && sv->pe5 && sv->x3e && sv->pa && sv->wt && sv->wn &&
                    sv->prow && sv->hid && sv->vpe && sv->hc1 && sv->hc2 && sv->hc3 && sv->vmask && sv->mask,
                "aggregate train: null saved array");
  PNR_CHECK_ARG((((uintptr_t)sv->h1 | (uintptr_t)sv->h2 | (uintptr_t)sv->h3 | (uintptr_t)sv->h4 |
                  (uintptr_t)sv->hid | (uintptr_t)sv->hc1 | (uintptr_t)sv->hc2 | (uintptr_t)sv->hc3) & 15) == 0,
                "aggregate train: saved activations must be 16-B aligned");
  return PNR_OK;
}

static bool scale_ok(float v) { return v > 0.f && v < 1e30f; }

// One validator per pack struct; `who` is the calling entry point's message prefix.
static int check_split_x3(const char* who, const pnr_mlp_x3* wx) {
  PNR_CHECK_ARG(wx && wx->w1bx && wx->w2x && wx->w3x && wx->w4x, "%s: null split weight pack", who);
  PNR_CHECK_ARG((((uintptr_t)wx->w1bx | (uintptr_t)wx->w2x | (uintptr_t)wx->w3x | (uintptr_t)wx->w4x) & 15) == 0,
                "%s: split packs must be 16-B aligned", who);
  return PNR_OK;
}

static int check_split_h2(const char* who, const pnr_mlp_h2* wh) {
  PNR_CHECK_ARG(wh && wh->w1bh && wh->w2h && wh->w3h && wh->w4h, "%s: null split weight pack", who);
  PNR_CHECK_ARG((((uintptr_t)wh->w1bh | (uintptr_t)wh->w2h | (uintptr_t)wh->w3h | (uintptr_t)wh->w4h) & 15) == 0,
                "%s: split packs must be 16-B aligned", who);
  for (int i = 0; i < 4; ++i) PNR_CHECK_ARG(scale_ok(wh->scale[i]), "%s: bad layer scale %d", who, i);
  return PNR_OK;
}

static int check_p1_h2(const char* who, const pnr_mlp_h2* wh) {
  PNR_CHECK_ARG(wh->w1ah && ((uintptr_t)wh->w1ah & 15) == 0 && scale_ok(wh->scale1a),
                "%s: bad block1.0 point-half pack", who);
  return PNR_OK;
}

static bool colour_packs_h2(const pnr_mlp_h2* wh) { return wh->wc1a && wh->wc1b && wh->wc2h && wh->wc3h; }

static int check_colour_h2(const char* who, const pnr_mlp_h2* wh) {
  PNR_CHECK_ARG((((uintptr_t)wh->wc1a | (uintptr_t)wh->wc1b | (uintptr_t)wh->wc2h | (uintptr_t)wh->wc3h) & 15) == 0,
                "%s: colour packs must be 16-B aligned", who);
  for (int i = 0; i < 3; ++i) PNR_CHECK_ARG(scale_ok(wh->cscale[i]), "%s: bad colour layer scale %d", who, i);
  return PNR_OK;
}

// ---------------------------------------------------------------------------
// The forward plan.  An entry point states what it is (FwdCall); the checks,
// the one AggArgs fill and the stage sequence follow from that here and
// nowhere else (DESIGN.md section 22 has the stage table).
enum class Arith { F32, X3, H2 };   // the per-pair chain: k_pairs, k_pairs_x3, k_pairs_h2

enum : unsigned { kMasked = 1, kTrain = 2, kGuarded = 4 };
struct FwdCall {
  const char* who;              // message prefix
  Arith arith;
  unsigned flags;               // kMasked: PointAggregator.forward mirror (pair_mask, no pidx); kTrain: keeps the
                                // backward's activations in `saved`; kGuarded: h2 training, fp32 rerun behind the flag
  const pnr_mlp_x3* wx;         // Arith::X3
  const pnr_mlp_h2* wh;         // Arith::H2
  const uint8_t* pair_mask;     // kMasked
  const pnr_agg_saved* saved;   // kTrain
  float* p1_table;              // the _p1 entry points: P1 lives here, not at the head of the scratch
  bool train() const { return flags & kTrain; }
};

// wh's optional packs (w1ah: P1 on k_point_pre_h2; wc1a..wc3h: the colour branch
// on k_color_h2).  A partial colour set is an error for the inference call and
// selects the fp32 colour branch for the training calls (pnr.h).
static int check_optional_h2(const FwdCall& c) {
  int rc;
  if (c.wh->w1ah) {
    if ((rc = check_p1_h2(c.who, c.wh))) return rc;
    PNR_CHECK_ARG(!c.train() || ((uintptr_t)c.saved->x1 & 15) == 0, "%s: saved x1 must be 16-B aligned", c.who);
  }
  PNR_CHECK_ARG(c.train() || !c.wh->wc1a || colour_packs_h2(c.wh), "%s: partial colour-branch packs", c.who);
  return colour_packs_h2(c.wh) ? check_colour_h2(c.who, c.wh) : PNR_OK;
}

static int aggregate_forward(const FwdCall& c, const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                             float* out_feat, float* out_weight, float* out_conf, void* scratch,
                             size_t scratch_bytes, void* stream) {
  int rc;
  const bool h2 = c.arith == Arith::H2, guarded = c.flags & kGuarded;
  // ---- every refusal, before the first launch
  PNR_CHECK_ARG(!guarded || (c.wh && c.wh->range_flag), "%s: range_flag required", c.who);
  if ((rc = check_common(pts, s, w, out_feat, scratch, scratch_bytes, c.p1_table))) return rc;
  if (c.train()) PNR_CHECK_DEFAULT_DIMS(c.who, pts, w);   // the training kernels: E = 32, order 2
  if (c.train() && (rc = check_saved(c.saved))) return rc;
  if (c.flags & kMasked) {
    PNR_CHECK_ARG(c.pair_mask, "%s: null pair_mask", c.who);
    PNR_CHECK_ARG(pts->pers, "%s: pers required", c.who);
    PNR_CHECK_ARG(s->pidx == nullptr, "%s: pidx must be NULL (identity rows)", c.who);
  } else {
    PNR_CHECK_ARG(pts->pers || (pts->campos && pts->camrot), "%s: need pers or camera", c.who);
  }
  if (c.arith != Arith::F32) {
    PNR_CHECK_ARG(s->pidx, "%s: pidx required", c.who);
    if ((rc = h2 ? check_split_h2(c.who, c.wh) : check_split_x3(c.who, c.wx))) return rc;
    PNR_CHECK_ARG(w->neg_slope >= 0.f && w->neg_slope <= 1.f, "%s: LeakyReLU slope must be in [0, 1]", c.who);
  }
  // the inference call checks the optional h2 packs for an empty sample list too, the
  // training calls only with samples, as they always have
  if (h2 && !c.train() && (rc = check_optional_h2(c))) return rc;
  if (s->n_max <= 0) return PNR_OK;
  if (h2 && c.train() && (rc = check_optional_h2(c))) return rc;

  // ---- the arguments
  AggArgs a{};
  a.pts = *pts;
  a.s = *s;
  a.w = *w;
  int32_t* const tile_ctr = carve(a, scratch, s->n_max, pts->used ? pts->n_used : pts->n, c.p1_table);
  if (c.train()) {   // hid / vmask are kept for the backward
    a.sv = *c.saved;
    a.hid = c.saved->hid;
    a.vmask = c.saved->vmask;
  }
  a.out_feat = out_feat;
  a.out_weight = out_weight;
  a.out_conf = out_conf;
  a.pair_mask = c.pair_mask;
  hipStream_t st = as_stream(stream);
  auto fp32 = [&](const AggArgs& x, int stages) {
    return c.train() ? launch_t<true>(x, st, stages) : launch_t<false>(x, st, stages);
  };
  // agg_intrp_order 1 (inference only, checked above): k_tail_o1 behind the colour kernel.
  // planes: hid still in k_pairs_h2's f16-split planes (the colour branch ran on k_color_h2)
  auto tail = [&](int rc0, bool planes) {
    if (rc0 || w->intrp_order != 1) return rc0;
    return launch_tail_o1(a.s, a.w, a.hid, planes, a.vmask, out_feat, st);
  };
  // point_features_dim != 32 (inference only): P1 from the wide per-point kernels
  // (aggregate_wide.hip, k_point_pre_h2_w); every later stage reads P1 rows only
  const bool wide = emb_width(*pts) != kEmb;

  // ---- the stages
  if (c.arith == Arith::F32) {   // k_point_pre -> k_pairs -> k_color
    if (!wide) return tail(fp32(a, kStageAll), false);
    if (!a.pts.p1_ready && (rc = launch_point_pre_w(a.pts, w->w1af, a.p1, st))) return rc;
    return tail(fp32(a, kStagePairs | kStageColor), false);
  }
  // P1: k_point_pre_h2 with wh->w1ah, else the fp32 k_point_pre; skipped on pts->p1_ready
  if (wide) {
    if (a.pts.p1_ready) rc = PNR_OK;
    else if (h2 && c.wh->w1ah)
      rc = launch_point_pre_h2_w(a.pts, c.wh->w1ah, c.wh->scale1a, c.wh->range_flag, a.p1, st);
    else rc = launch_point_pre_w(a.pts, w->w1af, a.p1, st);
    if (rc) return rc;
  } else if (h2 && c.wh->w1ah) {
    if ((c.train() || !a.pts.p1_ready) &&
        (rc = launch_point_pre_h2(a.pts, c.wh->w1ah, c.wh->scale1a, c.wh->range_flag, a.p1, st,
                                  c.train() ? c.saved->x1 : nullptr)))
      return rc;
  } else if ((rc = launch_t<false>(a, st, kStagePre))) {
    return rc;
  }
  // pairs: k_pairs_x3 / k_pairs_h2 (aggregate_x3.hip), with the training saves when `saved` is set
  if (h2) {
    const SplitW sw = {{c.wh->w1bh, c.wh->w2h, c.wh->w3h, c.wh->w4h},
                       {c.wh->scale[0], c.wh->scale[1], c.wh->scale[2], c.wh->scale[3]},
                       c.wh->range_flag};
    rc = launch_pairs_split<true>(a.pts, a.s, a.w, sw, a.p1, a.hid, a.vmask, out_feat, out_weight, out_conf,
                                  tile_ctr, st, c.saved);
  } else {
    const SplitW sw = {{c.wx->w1bx, c.wx->w2x, c.wx->w3x, c.wx->w4x}, {1.f, 1.f, 1.f, 1.f}, nullptr};
    rc = launch_pairs_split<false>(a.pts, a.s, a.w, sw, a.p1, a.hid, a.vmask, out_feat, out_weight, out_conf,
                                   tile_ctr, st, c.saved);
  }
  if (rc) return rc;
  // guarded: the native-fp32 chain over the same outputs, run on the device only if the flag is up
  AggArgs f = a;
  if (guarded) {
    f.run_if = c.wh->range_flag;
    AggArgs p = f;
    p.pts.p1_ready = c.wh->w1ah ? 0 : 1;   // P1 again on fp32 when k_point_pre_h2 made it
    if ((rc = launch_t<true>(p, st, kStagePre | kStagePairs))) return rc;
  }
  // colour: k_color_h2 with the colour packs (and, guarded, its fp32 rerun behind it), else k_color
  if (h2 && colour_packs_h2(c.wh)) {
    const void* cp[4] = {c.wh->wc1a, c.wh->wc1b, c.wh->wc2h, c.wh->wc3h};
    rc = launch_color_h2(a.s, a.w, cp, c.wh->cscale, c.wh->range_flag, a.hid, a.vmask, out_feat, st, a.pts.rw2c,
                         c.saved);
    return rc || !guarded ? tail(rc, true) : launch_t<true>(f, st, kStageColor);
  }
  // the inference k_pairs_h2 leaves hid as f16-split planes (k_color_h2's input): rows for k_color
  if (h2 && !c.train() && (rc = launch_hid_rows_h2(a.hid, s->n_max, st))) return rc;
  return tail(fp32(a, kStageColor), false);
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_aggregate_scratch_bytes(int64_t n_max, int64_t n_points, size_t* out) {
  PNR_CHECK_ARG(out && n_max >= 0 && n_points >= 0, "aggregate_scratch_bytes: bad args");
  *out = scratch_need(n_max, n_points);
  return PNR_OK;
}

extern "C" int pnr_aggregate_fwd(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                 float* out_feat, float* out_weight, float* out_conf, void* scratch,
                                 size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate", Arith::F32, 0, nullptr, nullptr, nullptr, nullptr};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_x3(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                    const pnr_mlp_x3* wx, float* out_feat, float* out_weight, float* out_conf,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate_x3", Arith::X3, 0, wx, nullptr, nullptr, nullptr};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_h2(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                    const pnr_mlp_h2* wh, float* out_feat, float* out_weight, float* out_conf,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate_h2", Arith::H2, 0, nullptr, wh, nullptr, nullptr};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

// The three inference calls with P1 in a table of the caller's (pnr.h, ABI 33).
static int check_p1_table(const char* who, const float* p1_table) {
  PNR_CHECK_ARG(p1_table, "%s: null p1_table", who);
  return PNR_OK;
}

extern "C" int pnr_aggregate_fwd_p1(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w, float* p1_table,
                                    float* out_feat, float* out_weight, float* out_conf, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  if (int rc = check_p1_table("aggregate_p1", p1_table)) return rc;
  const FwdCall c{"aggregate_p1", Arith::F32, 0, nullptr, nullptr, nullptr, nullptr, p1_table};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_x3_p1(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                       const pnr_mlp_x3* wx, float* p1_table, float* out_feat, float* out_weight,
                                       float* out_conf, void* scratch, size_t scratch_bytes, void* stream) {
  if (int rc = check_p1_table("aggregate_x3_p1", p1_table)) return rc;
  const FwdCall c{"aggregate_x3_p1", Arith::X3, 0, wx, nullptr, nullptr, nullptr, p1_table};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_h2_p1(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                       const pnr_mlp_h2* wh, float* p1_table, float* out_feat, float* out_weight,
                                       float* out_conf, void* scratch, size_t scratch_bytes, void* stream) {
  if (int rc = check_p1_table("aggregate_h2_p1", p1_table)) return rc;
  const FwdCall c{"aggregate_h2_p1", Arith::H2, 0, nullptr, wh, nullptr, nullptr, p1_table};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_point_pre_h2(const pnr_points* pts, const pnr_mlp_h2* wh, void* scratch, size_t scratch_bytes,
                                void* stream) {
  int rc;
  PNR_CHECK_ARG(pts && wh && pts->emb && scratch, "point_pre_h2: null pointer");
  if ((rc = check_p1_h2("point_pre_h2", wh))) return rc;
  PNR_CHECK_ARG(pts->emb_dim >= 0 && pts->emb_dim <= 64, "point_pre_h2: emb_dim %d unsupported (1..64, 0 = 32)",
                pts->emb_dim);
  const bool wide = emb_width(*pts) != kEmb;
  PNR_CHECK_ARG(((uintptr_t)pts->emb & (wide ? 3 : 15)) == 0 && ((uintptr_t)scratch & 15) == 0,
                "point_pre_h2: emb and scratch must be 16-B aligned (emb: 4-B with emb_dim != 32)");
  const int64_t n_p1 = pts->used ? pts->n_used : pts->n;
  PNR_CHECK_ARG(n_p1 >= 0 && scratch_bytes >= (size_t)(n_p1 > 0 ? n_p1 : 1) * kHid * sizeof(float),
                "point_pre_h2: scratch too small for the P1 rows");
  if (n_p1 == 0) return PNR_OK;
  if (wide)
    return launch_point_pre_h2_w(*pts, wh->w1ah, wh->scale1a, wh->range_flag, static_cast<float*>(scratch),
                                 as_stream(stream));
  return launch_point_pre_h2(*pts, wh->w1ah, wh->scale1a, wh->range_flag, static_cast<float*>(scratch),
                             as_stream(stream));
}

extern "C" int pnr_aggregate_fwd_masked(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                        const uint8_t* pair_mask, float* out_feat, float* out_weight,
                                        float* out_conf, void* scratch, size_t scratch_bytes,
                                        void* stream) {
  const FwdCall c{"aggregate_masked", Arith::F32, kMasked, nullptr, nullptr, pair_mask, nullptr};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_train(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                       const pnr_agg_saved* saved, float* out_feat, float* out_weight,
                                       float* out_conf, void* scratch, size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate_train", Arith::F32, kTrain, nullptr, nullptr, nullptr, saved};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_train_x3(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                          const pnr_mlp_x3* wx, const pnr_agg_saved* saved, float* out_feat,
                                          float* out_weight, float* out_conf, void* scratch, size_t scratch_bytes,
                                          void* stream) {
  const FwdCall c{"aggregate_train_x3", Arith::X3, kTrain, wx, nullptr, nullptr, saved};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_train_h2(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                          const pnr_mlp_h2* wh, const pnr_agg_saved* saved, float* out_feat,
                                          float* out_weight, float* out_conf, void* scratch, size_t scratch_bytes,
                                          void* stream) {
  const FwdCall c{"aggregate_train_h2", Arith::H2, kTrain, nullptr, wh, nullptr, saved};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_train_h2_guarded(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                                  const pnr_mlp_h2* wh, const pnr_agg_saved* saved,
                                                  float* out_feat, float* out_weight, float* out_conf,
                                                  void* scratch, size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate_train_h2_guarded", Arith::H2, kTrain | kGuarded, nullptr, wh, nullptr, saved};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}

extern "C" int pnr_aggregate_fwd_train_masked(const pnr_points* pts, const pnr_samples* s, const pnr_mlp* w,
                                              const uint8_t* pair_mask, const pnr_agg_saved* saved,
                                              float* out_feat, float* out_weight, float* out_conf,
                                              void* scratch, size_t scratch_bytes, void* stream) {
  const FwdCall c{"aggregate_train_masked", Arith::F32, kMasked | kTrain, nullptr, nullptr, pair_mask, saved};
  return aggregate_forward(c, pts, s, w, out_feat, out_weight, out_conf, scratch, scratch_bytes, stream);
}
