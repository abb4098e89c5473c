// The quad-row LDS pipeline shared by k_pairs, k_color (aggregate.hip) and
// k_pairs_bwd (aggregate_bwd.hip): the tile constants, the quad-row addressing
// and the fp32 MFMA layer over it with its weight-fragment ring.
#pragma once
#include "agg_common.h"

namespace pnr {

constexpr int kPackPad = 8;        // zero k-steps padded onto every packed weight matrix
                                   // (>= every prefetch depth, so prefetch never overruns)

// NT tiles of this wave out of NTOT tiles per k-step in the packed layout
// (p already points at this wave's first tile).
template <int NT, int NTOT = NT>
__device__ __forceinline__ void load_w(float (&a)[NT], const float* __restrict__ p, int t) {
#pragma unroll
  for (int T = 0; T < NT; ++T) a[T] = p[(t * NTOT + T) * 64];
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS layout of a 64-pair tile's layer input X^T (quad rows): neuron / input row n
// of pair column c lives at (n >> 2) * kQP + 4c + perm(n & 3) with
// perm = {0, 2, 1, 3}.  Then
//   * the MFMA B operand of k-steps t, t+1 (rows 2t+h, 2t+2+h for lane half
//     h) is ONE ds_read_b64 at (t >> 1) * kQP + 4c + 2h (t even), and
//   * an accumulator quad (rows 8q + 4h + 0..3 of a tile) is ONE
//     ds_write_b128,
// both conflict-free; kQP = 260 keeps the tail's row-strided b128 reads
// conflict-free too.
constexpr int kTP = 64;                 // pairs per tile
constexpr int kTS = kTP / kKN;          // samples per tile
constexpr int kQP = 4 * kTP + 4;        // floats per quad row
constexpr int kQD = 4;                  // k_pairs weight prefetch depth (k-steps)

__device__ __forceinline__ constexpr int qperm(int i) { return ((i & 1) << 1) | (i >> 1); }
__device__ __forceinline__ constexpr int qaddr(int n, int c) { return (n >> 2) * kQP + 4 * c + qperm(n & 3); }

// Issue the first kQD k-steps of a layer's weight fragments into the ring.
// Called as soon as the previous layer's last MFMA is issued (or before the
// gather for layer 1), so the L2 latency hides behind the layer boundary.
template <int NT, int NTOT = 8>
__device__ __forceinline__ void prime_q(float (&a)[kQD][NT], const float* __restrict__ wf, int lane) {
#pragma unroll
  for (int d = 0; d < kQD; ++d) load_w<NT, NTOT>(a[d], wf + lane, d);
}

// Y^T += W . X^T for NT neuron tiles x PT 32-pair halves over nsteps k-steps.
// Weight fragments kQD steps ahead in a register ring (primed by prime_q);
// the next kQD steps' B operands read from LDS one iteration ahead (kQD/2 b64
// per half).
template <int NT, int PT, int NTOT = 8>
__device__ __forceinline__ void mlp_layer_q(f32x16 (&acc)[PT * NT], float (&a)[kQD][NT],
                                            const float* __restrict__ wf, const float* X, int nsteps,
                                            int lane) {
  constexpr int D = kQD;
  const int c = lane & 31, h = lane >> 5;
  const float* p = wf + lane;
  const float* xr = X + 4 * c + 2 * h;
  float2 x[D / 2][PT];
#pragma unroll
  for (int i = 0; i < D / 2; ++i)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) x[i][pt] = *reinterpret_cast<const float2*>(xr + 128 * pt + i * kQP);
  auto step = [&](const float (&w)[NT], const float2 (&xx)[PT], bool hi) {
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int T = 0; T < NT; ++T)
        acc[pt * NT + T] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[T], hi ? xx[pt].y : xx[pt].x,
                                                                acc[pt * NT + T], 0, 0, 0);
  };
  int t = 0;
#pragma unroll 1
  for (; t + D <= nsteps; t += D) {
    const float* xn = xr + ((t + D) >> 1) * kQP;
    float2 y[D / 2][PT];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      step(a[d], x[d >> 1], d & 1);
      if (d == 0) {
#pragma unroll
        for (int i = 0; i < D / 2; ++i)
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) y[i][pt] = *reinterpret_cast<const float2*>(xn + 128 * pt + i * kQP);
      }
      load_w<NT, NTOT>(a[d], p, t + D + d);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < D / 2; ++i)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) x[i][pt] = y[i][pt];
  }
  const int rem = nsteps - t;  // 0..D-1
#pragma unroll
  for (int d = 0; d < D - 1; ++d)
    if (rem > d) step(a[d], x[d >> 1], d & 1);
}

constexpr int kPairWaves = 4;
constexpr int kNTW = 8 / kPairWaves;   // neuron tiles per wave
constexpr int kPTW = kTP / 32;         // 32-pair halves per tile

}  // namespace pnr
