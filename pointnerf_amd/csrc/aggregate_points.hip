// Per-point bookkeeping around the aggregate, none of it MFMA: neighbour-list
// counts (pnr_point_counts), the used-point list (pnr_used_points), the
// deterministic per-point sums of per-pair gradients (pnr_pairs_to_points(_ex),
// pnr_pairs_to_points_conf) and block1.0's point-half inputs (pnr_point_pe3*).
#include "agg_common.h"

namespace pnr {

// Per-point entry counts of a query's neighbour lists: counts[p] += 1 for every
// pidx entry p >= 0 of the first (*n_dev) samples (float atomics of integers:
// exact and order-free below 2^24).
__global__ void k_point_counts(const int32_t* __restrict__ pidx, const int32_t* __restrict__ n_dev, int K,
                               int64_t cap, float* __restrict__ counts) {
  int64_t ns = *n_dev;
  ns = ns < cap ? ns : cap;
  const int64_t n = ns * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t p = pidx[i];
    if (p >= 0) atomicAdd(counts + p, 1.f);
  }
}

// pnr_used_points: a byte per point marked by plain stores (20 MB at c5's 20 M
// points, where an int32 flag per point was 80 MB of randomly touched lines;
// bit atomics measured slower: each drops its line from the XCD's L2), packed
// to one bit per point with the words' popcounts, ranked by a scan of those.
// The read comes before the store: neighbouring samples share most points, so
// nearly every flag is already set and stays a cached read.
__global__ void k_mark_used(const int32_t* __restrict__ pidx, const int32_t* __restrict__ n_dev, int K, int64_t cap,
                            uint8_t* __restrict__ flags) {
  const int64_t n = (n_dev ? (int64_t)*n_dev : cap) * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t p = pidx[i];
    if (p >= 0 && flags[p] == 0) flags[p] = 1;
  }
}

// word w of the bitset from flags[32w .. 32w+32) (two 16-B loads; the byte array
// is padded to whole words), cnt[w] = its popcount
__global__ void k_pack_used(const uint8_t* __restrict__ flags, int64_t nw, uint32_t* __restrict__ bits,
                            int32_t* __restrict__ cnt) {
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
    const uint4* f = reinterpret_cast<const uint4*>(flags + w * 32);
    const uint4 a = f[0], b = f[1];
    const uint32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) m |= ((q[j] >> (8 * k)) & 1u) << (4 * j + k);
    bits[w] = m;
    cnt[w] = __popc(m);
  }
}

// used_map[p] = rank of p (word prefix + set bits below p in its word) or -1;
// used[rank] = p.
__global__ void k_used_list(const uint32_t* __restrict__ bits, const int32_t* __restrict__ wpre, int64_t n_points,
                            int32_t* __restrict__ used_map, int32_t* __restrict__ used) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_points;
       p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t word = bits[p >> 5];
    const int b = (int)(p & 31);
    if ((word >> b) & 1u) {
      const int32_t r = wpre[p >> 5] + __popc(word & ((1u << b) - 1u));
      used_map[p] = r;
      used[r] = (int32_t)p;
    } else {
      used_map[p] = -1;
    }
  }
}

// Sum of a run of pairs sorted by point row, in pair order (deterministic):
// the run's positions are found 64 at a time with one ballot, the pair ids
// loaded one per lane and broadcast, and four dz1 rows read before they are
// added, so a wave keeps four row loads in flight instead of one.
template <bool EX>
__device__ __forceinline__ void run_sum(const int32_t* __restrict__ prow_sorted, const int32_t* __restrict__ pair_of,
                                        int64_t P, int64_t i, int32_t pr, const float* __restrict__ dz1,
                                        const float* __restrict__ g_pair, float4& s, float& ge) {
  const int lane = threadIdx.x & 63;
  bool first = true;
  for (int64_t j0 = i;; j0 += 64) {
    const int64_t jj = j0 + lane;
    const int32_t pl = jj < P ? prow_sorted[jj] : -2;
    const uint64_t same = __ballot(pl == pr);
    const int len = same == ~0ull ? 64 : __builtin_ctzll(~same);
    const int32_t mine = lane < len ? pair_of[jj] : 0;
    int t = 0;
    for (; t + 4 <= len; t += 4) {
      int64_t pq[4];
      float4 v[4];
      float gq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) pq[u] = __shfl(mine, t + u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = reinterpret_cast<const float4*>(dz1 + pq[u] * kHid)[lane];
        gq[u] = (EX && lane < 6) ? g_pair[pq[u] * 8 + lane] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (first && !EX) {
          s = v[u];
          first = false;
        } else {
          s.x += v[u].x;
          s.y += v[u].y;
          s.z += v[u].z;
          s.w += v[u].w;
        }
        if (EX && lane < 6) ge += gq[u];
      }
    }
    for (; t < len; ++t) {
      const int64_t pq = __shfl(mine, t);
      const float4 v = reinterpret_cast<const float4*>(dz1 + pq * kHid)[lane];
      if (first && !EX) {
        s = v;
        first = false;
      } else {
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
      }
      if (EX && lane < 6) ge += g_pair[pq * 8 + lane];
    }
    if (len < 64) break;
  }
}

// A run that ends inside the caller's 64-position chunk: its pair ids are the
// chunk's lanes l .. l + len - 1 (`mine`), so only the dz1 rows are loaded.
template <bool EX>
__device__ __forceinline__ void run_sum_chunk(int32_t mine, int l, int len, const float* __restrict__ dz1,
                                              const float* __restrict__ g_pair, float4& s, float& ge) {
  const int lane = threadIdx.x & 63;
  int t = 0;
  for (; t + 4 <= len; t += 4) {
    int64_t pq[4];
    float4 v[4];
    float gq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pq[u] = __shfl(mine, l + t + u);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = reinterpret_cast<const float4*>(dz1 + pq[u] * kHid)[lane];
      gq[u] = (EX && lane < 6) ? g_pair[pq[u] * 8 + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (t + u == 0 && !EX) {
        s = v[u];
      } else {
        s.x += v[u].x;
        s.y += v[u].y;
        s.z += v[u].z;
        s.w += v[u].w;
      }
      if (EX && lane < 6) ge += gq[u];
    }
  }
  for (; t < len; ++t) {
    const int64_t pq = __shfl(mine, l + t);
    const float4 v = reinterpret_cast<const float4*>(dz1 + pq * kHid)[lane];
    if (t == 0 && !EX) {
      s = v;
    } else {
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    if (EX && lane < 6) ge += g_pair[pq * 8 + lane];
  }
}

// d P1 rows from dz1 without atomics: pairs sorted by point row (stable, so
// each point's pairs in pair order -- a deterministic sum); one wave per run of
// equal rows, lane = 4 neurons (float4).
__global__ void k_pairs_to_points(const int32_t* __restrict__ prow_sorted, const int32_t* __restrict__ pair_of,
                                  int64_t P, const float* __restrict__ dz1, const int32_t* __restrict__ used_map,
                                  float* __restrict__ d_p1, uint32_t* __restrict__ absmax) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  __shared__ unsigned bmax;
  if (threadIdx.x == 0) bmax = 0u;
  __syncthreads();
  unsigned mb = 0u;   // max |d_p1| of this lane's rows (float bits: NaN propagates)
  // 64 sorted positions per wave and step: one ballot finds the runs that start there
  for (int64_t i0 = (blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6)) * 64; i0 < P; i0 += waves * 64) {
    const int64_t ii = i0 + lane;
    const int32_t pr_l = ii < P ? prow_sorted[ii] : -1;
    const int32_t pv_l = ii > 0 && ii < P ? prow_sorted[ii - 1] : -1;
    const int32_t mine = ii < P ? pair_of[ii] : 0;
    uint64_t starts = __ballot(pr_l >= 0 && (ii == 0 || pv_l != pr_l));
    const uint64_t bounds = __ballot(ii >= P || ii == 0 || pv_l != pr_l);   // a new value (or the end) begins
    while (starts) {
      const int l = __builtin_ctzll(starts);
      starts &= starts - 1;
      const int64_t i = i0 + l;
      const int32_t pr = __shfl(pr_l, l);
      const uint64_t after = l == 63 ? 0ull : bounds & (~0ull << (l + 1));
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      float ge = 0.f;
      if (after) run_sum_chunk<false>(mine, l, __builtin_ctzll(after) - l, dz1, nullptr, s, ge);
      else run_sum<false>(prow_sorted, pair_of, P, i, pr, dz1, nullptr, s, ge);   // runs past the chunk
      reinterpret_cast<float4*>(d_p1 + (used_map ? (int64_t)used_map[pr] : (int64_t)pr) * kHid)[lane] = s;
      mb = max(max(mb, max(__float_as_uint(fabsf(s.x)), __float_as_uint(fabsf(s.y)))),
               max(__float_as_uint(fabsf(s.z)), __float_as_uint(fabsf(s.w))));
    }
  }
  if (absmax) {
    wave_absmax_to(&bmax, mb);
    __syncthreads();
    if (threadIdx.x == 0 && bmax) atomicMax(absmax, bmax);
  }
}

// pnr_pairs_to_points_ex: k_pairs_to_points plus the per-point sums of g_pair
// (lanes 0..5 of the run's wave): d_color[p] = sum g[0..2], d_dir[p] =
// Rw_p^T sum g[3..5] (Rw_p: the point's per-point Rw2c or the uniform one).
// Written, not added: every referenced point's rows, deterministic.
__global__ void k_pairs_to_points_ex(const int32_t* __restrict__ prow_sorted, const int32_t* __restrict__ pair_of,
                                     int64_t P, const float* __restrict__ dz1, const int32_t* __restrict__ used_map,
                                     float* __restrict__ d_p1, uint32_t* __restrict__ absmax,
                                     const float* __restrict__ g_pair, const float* __restrict__ rw_uniform,
                                     const float* __restrict__ rw_pp, float* __restrict__ d_color,
                                     float* __restrict__ d_dir) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  __shared__ unsigned bmax;
  if (threadIdx.x == 0) bmax = 0u;
  __syncthreads();
  unsigned mb = 0u;
  // 64 sorted positions per wave and step: one ballot finds the runs that start there
  for (int64_t i0 = (blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6)) * 64; i0 < P; i0 += waves * 64) {
    const int64_t ii = i0 + lane;
    const int32_t pr_l = ii < P ? prow_sorted[ii] : -1;
    const int32_t pv_l = ii > 0 && ii < P ? prow_sorted[ii - 1] : -1;
    const int32_t mine = ii < P ? pair_of[ii] : 0;
    uint64_t starts = __ballot(pr_l >= 0 && (ii == 0 || pv_l != pr_l));
    const uint64_t bounds = __ballot(ii >= P || ii == 0 || pv_l != pr_l);   // a new value (or the end) begins
    while (starts) {
      const int l = __builtin_ctzll(starts);
      starts &= starts - 1;
      const int64_t i = i0 + l;
      const int32_t pr = __shfl(pr_l, l);
      const uint64_t after = l == 63 ? 0ull : bounds & (~0ull << (l + 1));
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      float ge = 0.f;   // lane e < 6: sum of g_pair[.][e]
      if (after) run_sum_chunk<true>(mine, l, __builtin_ctzll(after) - l, dz1, g_pair, s, ge);
      else run_sum<true>(prow_sorted, pair_of, P, i, pr, dz1, g_pair, s, ge);   // runs past the chunk
      reinterpret_cast<float4*>(d_p1 + (used_map ? (int64_t)used_map[pr] : (int64_t)pr) * kHid)[lane] = s;
      mb = max(max(mb, max(__float_as_uint(fabsf(s.x)), __float_as_uint(fabsf(s.y)))),
               max(__float_as_uint(fabsf(s.z)), __float_as_uint(fabsf(s.w))));
      const float g3 = __shfl(ge, 3), g4 = __shfl(ge, 4), g5 = __shfl(ge, 5);
      if (lane < 3) {
        if (d_color) d_color[(int64_t)pr * 3 + lane] = ge;
        if (d_dir) {   // d dir_a = sum_j Rw[j][a] gd_j
          const float* R = rw_pp ? rw_pp + (int64_t)pr * 9 : rw_uniform;
          const float r0 = R ? R[lane] : (lane == 0 ? 1.f : 0.f);
          const float r1 = R ? R[3 + lane] : (lane == 1 ? 1.f : 0.f);
          const float r2 = R ? R[6 + lane] : (lane == 2 ? 1.f : 0.f);
          d_dir[(int64_t)pr * 3 + lane] = r0 * g3 + r1 * g4 + r2 * g5;
        }
      }
    }
  }
  if (absmax) {
    wave_absmax_to(&bmax, mb);
    __syncthreads();
    if (threadIdx.x == 0 && bmax) atomicMax(absmax, bmax);
  }
}

// X1[p] = [emb, PE_3(emb)] (networks.py:175-190: channel d, band f -> 32 + 2(3d+f) + {sin, cos})
__global__ void k_point_pe3(const float* __restrict__ emb, const int32_t* __restrict__ rows, int64_t n,
                            float* __restrict__ x1) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n * kEmb;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / kEmb;
    const int d = (int)(i - p * kEmb);
    const float e = emb[(rows ? (int64_t)rows[p] : p) * kEmb + d];   // rows: the used points (a gather)
    float* o = x1 + p * 224;
    o[d] = e;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      float sn, cs;
      sincosf(e * (float)(1 << f), &sn, &cs);
      o[kEmb + 2 * (3 * d + f)] = sn;
      o[kEmb + 2 * (3 * d + f) + 1] = cs;
    }
  }
}

__global__ void k_point_pe3_bwd(const float* __restrict__ emb, const int32_t* __restrict__ rows,
                                const float* __restrict__ dx1, int64_t n, float* __restrict__ d_emb) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n * kEmb;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / kEmb;
    const int d = (int)(i - p * kEmb);
    const int64_t t = (rows ? (int64_t)rows[p] : p) * kEmb + d;   // rows: scatter into the full table
    const float e = emb[t];
    const float* g = dx1 + p * 224;
    float acc = g[d];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const float b = (float)(1 << f);
      float sn, cs;
      sincosf(e * b, &sn, &cs);
      acc += b * (cs * g[kEmb + 2 * (3 * d + f)] - sn * g[kEmb + 2 * (3 * d + f) + 1]);
    }
    d_emb[t] += acc;
  }
}

// d conf per point from k_pairs_bwd's per-pair terms: the thread at the first
// sorted position of a point's run adds the run's terms in pair order (eight
// loads in flight), so the sum has one order -- bitwise repeatable.
__global__ void __launch_bounds__(256) k_conf_from_runs(const int32_t* __restrict__ prow_sorted,
                                                        const int32_t* __restrict__ pair_of, int64_t P,
                                                        const float* __restrict__ dconf_pair,
                                                        float* __restrict__ d_conf) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += stride) {
    const int32_t pr = prow_sorted[i];
    if (pr < 0 || (i > 0 && prow_sorted[i - 1] == pr)) continue;
    float s = 0.f;
    int64_t j = i;
    bool more = true;
    while (more) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool in = j + u < P && prow_sorted[j + u] == pr;   // a run is contiguous: once false, false
        v[u] = in ? dconf_pair[pair_of[j + u]] : 0.f;
        if (!in) more = false;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];   // + 0.f past the run's end changes nothing
      j += 8;
    }
    d_conf[pr] = s;
  }
}
}  // namespace pnr

using namespace pnr;

// flags: the bytes [32 * nw] | the bitset [nw] (fits the caller's int32 [n_points]
// only from 64 points up: below, both live in scratch); scratch: the word prefix
// [nw + 1] | (small n: bytes + bits) | the scan's scratch, each 16-B padded
static size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }
static bool used_small(int64_t n_points) { return cdiv(n_points, 32) * 36 > n_points * 4; }
static size_t used_head_bytes(int64_t n_points) {
  const int64_t nw = cdiv(n_points, 32);
  return pad16((size_t)(nw + 1) * 4) + (used_small(n_points) ? pad16((size_t)nw * 36) : 0);
}

extern "C" int pnr_used_points_scratch_bytes(int64_t n_points, size_t* out) {
  PNR_CHECK_ARG(out && n_points >= 0, "used_points_scratch_bytes: bad args");
  *out = used_head_bytes(n_points) + scan_scratch_bytes(cdiv(n_points, 32));
  return PNR_OK;
}

extern "C" int pnr_used_points(const int32_t* pidx, const int32_t* n_samples_dev, int32_t K, int64_t cap_samples,
                               int64_t n_points, int32_t* flags, int32_t* used_map, int32_t* used, int32_t* n_used_dev,
                               void* scratch, size_t scratch_bytes, void* stream) {
  PNR_CHECK_ARG(pidx && flags && used_map && used && n_used_dev && scratch && K > 0 && cap_samples >= 0 &&
                    n_points > 0, "used_points: bad args");
  const int64_t nw = cdiv(n_points, 32);
  const size_t hb = used_head_bytes(n_points);
  PNR_CHECK_ARG(scratch_bytes >= hb + scan_scratch_bytes(nw), "used_points: scratch too small (%zu < %zu)",
                scratch_bytes, hb + scan_scratch_bytes(nw));
  PNR_CHECK_ARG(((uintptr_t)flags & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
                "used_points: flags / scratch must be 16-B aligned");
  hipStream_t st = as_stream(stream);
  int32_t* wpre = static_cast<int32_t*>(scratch);
  uint8_t* bytes = used_small(n_points) ? static_cast<uint8_t*>(scratch) + pad16((size_t)(nw + 1) * 4)
                                        : reinterpret_cast<uint8_t*>(flags);
  uint32_t* bits = reinterpret_cast<uint32_t*>(bytes + nw * 32);
  PNR_HIP(hipMemsetAsync(bytes, 0, (size_t)nw * 32, st));
  if (cap_samples > 0) {
    hipLaunchKernelGGL(k_mark_used, dim3(grid_for(cap_samples * K, 256)), dim3(256), 0, st, pidx, n_samples_dev, K,
                       cap_samples, bytes);
    PNR_LAUNCH_CHECK();
  }
  // the words' popcounts go through `used` (n_points >= nw entries, written after)
  hipLaunchKernelGGL(k_pack_used, dim3(grid_for(nw, 256)), dim3(256), 0, st, bytes, nw, bits, used);
  PNR_LAUNCH_CHECK();
  int rc;
  if ((rc = exclusive_scan(used, nw, nullptr, wpre, nw + 1, n_used_dev, static_cast<char*>(scratch) + hb,
                           scratch_bytes - hb, st, 0)))
    return rc;
  hipLaunchKernelGGL(k_used_list, dim3(grid_for(n_points, 256)), dim3(256), 0, st, bits, wpre, n_points, used_map,
                     used);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_pairs_to_points_ex(const int32_t* prow_sorted, const int32_t* pair_of, int64_t P,
                                      const float* dz1, const int32_t* used_map, float* d_p1, uint32_t* d_p1_absmax,
                                      const float* g_pair, const float* rw_uniform, const float* rw_pp,
                                      float* d_color, float* d_dir, void* stream) {
  PNR_CHECK_ARG(P >= 0 && (P == 0 || (prow_sorted && pair_of && dz1 && d_p1 && g_pair)),
                "pairs_to_points_ex: bad args");
  PNR_CHECK_ARG((((uintptr_t)dz1 | (uintptr_t)d_p1) & 15) == 0, "pairs_to_points_ex: rows must be 16-B aligned");
  if (P == 0) return PNR_OK;
  hipLaunchKernelGGL(k_pairs_to_points_ex, dim3(grid_for(cdiv(P, 64), 4, 2048)), dim3(256), 0, as_stream(stream), prow_sorted,
                     pair_of, P, dz1, used_map, d_p1, d_p1_absmax, g_pair, rw_uniform, rw_pp, d_color, d_dir);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_point_counts(const int32_t* pidx, const int32_t* n_dev, int32_t K, int64_t cap, float* counts,
                                void* stream) {
  PNR_CHECK_ARG(n_dev && K > 0 && cap >= 0 && (cap == 0 || (pidx && counts)), "point_counts: bad args");
  if (cap == 0) return PNR_OK;
  hipLaunchKernelGGL(k_point_counts, dim3(grid_for(cap * K, 256, 2048)), dim3(256), 0, as_stream(stream), pidx,
                     n_dev, K, cap, counts);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_pairs_to_points(const int32_t* prow_sorted, const int32_t* pair_of, int64_t P, const float* dz1,
                                   const int32_t* used_map, float* d_p1, uint32_t* d_p1_absmax, void* stream) {
  PNR_CHECK_ARG(P >= 0 && (P == 0 || (prow_sorted && pair_of && dz1 && d_p1)), "pairs_to_points: bad args");
  PNR_CHECK_ARG((((uintptr_t)dz1 | (uintptr_t)d_p1) & 15) == 0, "pairs_to_points: rows must be 16-B aligned");
  if (P == 0) return PNR_OK;
  hipLaunchKernelGGL(k_pairs_to_points, dim3(grid_for(cdiv(P, 64), 4, 2048)), dim3(256), 0, as_stream(stream), prow_sorted,
                     pair_of, P, dz1, used_map, d_p1, d_p1_absmax);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_pairs_to_points_conf(const int32_t* prow_sorted, const int32_t* pair_of, int64_t P,
                                        const float* dconf_pair, float* d_conf, void* stream) {
  PNR_CHECK_ARG(P >= 0 && (P == 0 || (prow_sorted && pair_of && dconf_pair && d_conf)),
                "pairs_to_points_conf: bad args");
  if (P == 0) return PNR_OK;
  hipLaunchKernelGGL(k_conf_from_runs, dim3(grid_for(P, 256, 4096)), dim3(256), 0, as_stream(stream), prow_sorted,
                     pair_of, P, dconf_pair, d_conf);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_point_pe3(const float* emb, int64_t n, float* x1, void* stream) {
  PNR_CHECK_ARG(emb && x1 && n >= 0, "point_pe3: bad args");
  if (n == 0) return PNR_OK;
  hipLaunchKernelGGL(k_point_pe3, dim3(grid_for(n * kEmb, 256)), dim3(256), 0, as_stream(stream), emb, nullptr, n,
                     x1);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_point_pe3_bwd(const float* emb, const float* d_x1, int64_t n, float* d_emb, void* stream) {
  PNR_CHECK_ARG(emb && d_x1 && d_emb && n >= 0, "point_pe3_bwd: bad args");
  if (n == 0) return PNR_OK;
  hipLaunchKernelGGL(k_point_pe3_bwd, dim3(grid_for(n * kEmb, 256)), dim3(256), 0, as_stream(stream), emb, nullptr,
                     d_x1, n, d_emb);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_point_pe3_rows(const float* emb, const int32_t* rows, int64_t n, float* x1, void* stream) {
  PNR_CHECK_ARG(emb && rows && x1 && n >= 0, "point_pe3_rows: bad args");
  if (n == 0) return PNR_OK;
  hipLaunchKernelGGL(k_point_pe3, dim3(grid_for(n * kEmb, 256)), dim3(256), 0, as_stream(stream), emb, rows, n, x1);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_point_pe3_bwd_rows(const float* emb, const int32_t* rows, const float* d_x1, int64_t n,
                                      float* d_emb, void* stream) {
  PNR_CHECK_ARG(emb && rows && d_x1 && d_emb && n >= 0, "point_pe3_bwd_rows: bad args");
  if (n == 0) return PNR_OK;
  hipLaunchKernelGGL(k_point_pe3_bwd, dim3(grid_for(n * kEmb, 256)), dim3(256), 0, as_stream(stream), emb, rows,
                     d_x1, n, d_emb);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
