// The perspective-frustum point query: the reference's
// lighting_fast_querier of models/neural_points/query_point_indices.py
// (--wcoord_query 0): get_occ_vox, near_vox_full, insert_vox_points and
// query_neigh_along_ray_layered, restated without slot tables.
//
//   k_pq_bin      one thread per point: the floor cell sets a held bit (32-bit
//                 atomicOr), the truncation cell counts into its column
//   scan          column counts -> col_off
//   k_pq_scatter  (z, id) keys into the column's segment, in arrival order
//   k_pq_dilate   held bits -> occupied bits (the query_size block), one
//                 thread per (column, word); bits are z-contiguous per column
//   k_pq_records  one thread per listed point: its rank among its column's
//                 keys places its float4 record in (z, id) order; the P cap
//   k_pq_colstats one thread per column: held voxels
//   k_pq_select   one thread per ray: far_id > 0 from its column's words
//   scan          ray_mask -> compact row of every hit ray, R' on the device
//   k_pq_knn      one thread per (hit ray, slot): the slot-th occupied id, the
//                 centre, the layered walk over the neighbouring columns' runs
//
// The kernels up to k_pq_colstats depend on the camera and the cloud only
// (pq_build); the rest is per ray.  pnr_pquery_bufs is a second
// per-ray part on the same build, writing the world query's pnr_query_bufs
// instead of [R,SR,.] rows:
//   k_pq_columns  one thread per ray: ray_hit and n_filled = min(SR, occupied ids)
//   scan          n_filled -> ray_off, S_filled
//   k_pq_fill     one thread per (ray, slot < n_filled): pq_sample (k_pq_knn's
//                 walk), fill_rs, slot_d, pidx, sample_p, pers2w, vflag, ray_vcnt
//   scan          vflag -> valid_off + valid_list; ray_vcnt -> ray_row
//
// A ray's result depends on the cloud and its own pixel only (no pixel_map
// "first thread of the column" protocol), and no table is sized by the cell
// count: the bitmaps take 2 bits per cell, everything else is per point, per
// column or per ray.
//
// Arithmetic: the reference's fp32 operations in its order, one rounding each
// (this file is built with -ffp-contract=off); the centres go through double
// where the reference's `+ 0.5` literals promote them.  tests/pquery_ref.py
// restates all of it serially.
#include "pnr_common.h"

namespace pnr {

constexpr int kPqBlock = 256;
constexpr int kPqKnnBlock = 128;
constexpr int kPqMaxSize = 15;   // kernel_size / query_size per axis (the z dilation looks one word each way)

struct PqGeom {
  float shift[3], svs[3], rvs[3];
  int dims[3], vscale[3];
  int w, h;
  int wz;        // words of 32 depth bits per column
  int columns;   // dims[0] * dims[1]
};

// scratch layout (every part 16-byte aligned); the first `zero_bytes` are cleared per call
struct PqScratch {
  uint32_t* held;     // [columns * wz]
  uint32_t* occ;      // [columns * wz]
  int32_t* col_cnt;   // [columns + 1] points per column (truncation cell)
  int32_t* col_cur;   // [columns] scatter cursor
  size_t zero_bytes;
  int32_t* col_off;   // [columns + 1]
  int32_t* pcol;      // [N] truncation column or -1
  int32_t* pz;        // [N] truncation depth id
  uint64_t* keys;     // [N] z << 32 | id
  float4* rec;        // [N] X, Y, Z, bitcast(id)
  int32_t* rec_z;     // [N]
  int32_t* hit;       // [R] ray_mask as int32
  int32_t* ray_off;   // [R + 1]
  void* scan;         // max(scan(columns), scan(R))
  size_t scan_bytes;
  size_t total;
};

inline size_t al16(size_t b) { return (b + 15) / 16 * 16; }

inline PqScratch pq_layout(void* base, int64_t N, int64_t R, int64_t columns, int wz) {
  PqScratch s = {};
  char* p = static_cast<char*>(base);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + o : nullptr;
    o += al16(bytes);
    return (void*)q;
  };
  s.held = (uint32_t*)take((size_t)columns * wz * 4);
  s.occ = (uint32_t*)take((size_t)columns * wz * 4);
  s.col_cnt = (int32_t*)take((size_t)(columns + 1) * 4);
  s.col_cur = (int32_t*)take((size_t)columns * 4);
  s.zero_bytes = o;
  s.col_off = (int32_t*)take((size_t)(columns + 1) * 4);
  s.pcol = (int32_t*)take((size_t)(N > 0 ? N : 1) * 4);
  s.pz = (int32_t*)take((size_t)(N > 0 ? N : 1) * 4);
  s.keys = (uint64_t*)take((size_t)(N > 0 ? N : 1) * 8);
  s.rec = (float4*)take((size_t)(N > 0 ? N : 1) * 16);
  s.rec_z = (int32_t*)take((size_t)(N > 0 ? N : 1) * 4);
  s.hit = (int32_t*)take((size_t)(R > 0 ? R : 1) * 4);
  s.ray_off = (int32_t*)take((size_t)(R + 1) * 4);
  s.scan_bytes = al16(scan_scratch_bytes(columns > R ? columns : R));
  s.scan = take(s.scan_bytes);
  s.total = o;
  return s;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();
}

// One lane per wave adds the wave's count (a handful of atomics per block).
__device__ __forceinline__ void wave_count(int32_t* dst, bool flag) {
  const unsigned long long b = __ballot(flag);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(dst, (int)__popcll(b));
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// ------------------------------------------------------------------- bin
__global__ void __launch_bounds__(kPqBlock) k_pq_bin(const float* __restrict__ pers, int64_t N, PqGeom g,
                                                     uint32_t* held, int32_t* col_cnt, int32_t* pcol, int32_t* pz,
                                                     pnr_pquery_stats* stats) {
  const int64_t i = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  bool bad = false, in_floor = false;
  if (i < N) {
    const Row3 p = reinterpret_cast<const Row3*>(pers)[i];
    int col = -1, cz = 0;
    if (!finite3(p.x, p.y, p.z)) {
      bad = true;
    } else {
      // (p - shift) / vsize per axis: get_occ_vox floors it, insert_vox_points truncates it
      const float t0 = __fdiv_rn(__fsub_rn(p.x, g.shift[0]), g.svs[0]);
      const float t1 = __fdiv_rn(__fsub_rn(p.y, g.shift[1]), g.svs[1]);
      const float t2 = __fdiv_rn(__fsub_rn(p.z, g.shift[2]), g.svs[2]);
      const float d0 = (float)g.dims[0], d1 = (float)g.dims[1], d2 = (float)g.dims[2];
      if (!(fabsf(t0) < __builtin_inff() && fabsf(t1) < __builtin_inff() && fabsf(t2) < __builtin_inff())) {
        bad = true;   // a zero or overflowing quotient: no defined conversion
      } else {
        in_floor = t0 >= 0.f && t0 < d0 && t1 >= 0.f && t1 < d1 && t2 >= 0.f && t2 < d2;
        const bool in_trunc = t0 > -1.f && t0 < d0 && t1 > -1.f && t1 < d1 && t2 > -1.f && t2 < d2;
        if (in_floor) {   // non-negative: floor == truncation
          const int c = (int)t0 * g.dims[1] + (int)t1, z = (int)t2;
          atomicOr(held + (int64_t)c * g.wz + (z >> 5), 1u << (z & 31));
        }
        if (in_trunc) {
          col = (int)t0 * g.dims[1] + (int)t1;   // (int) of (-1, 0) is 0
          cz = (int)t2;
          atomicAdd(col_cnt + col, 1);
        }
      }
    }
    pcol[i] = col;
    pz[i] = cz;
  }
  wave_count(&stats->n_bad_points, bad);
  wave_count(&stats->n_points_in_grid, in_floor);
}

__global__ void __launch_bounds__(kPqBlock) k_pq_scatter(int64_t N, const int32_t* __restrict__ pcol,
                                                         const int32_t* __restrict__ pz,
                                                         const int32_t* __restrict__ col_off, int32_t* col_cur,
                                                         uint64_t* keys) {
  const int64_t i = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  if (i >= N) return;
  const int col = pcol[i];
  if (col < 0) return;
  const int at = col_off[col] + atomicAdd(col_cur + col, 1);   // < col_off[col + 1]: k_pq_bin counted this point
  keys[at] = ((uint64_t)(uint32_t)pz[i] << 32) | (uint32_t)i;
}

// ---------------------------------------------------------------- dilate
// A held voxel c marks [c - q/2, c + (q+1)/2) per axis, so cell t is occupied
// when a voxel of [t - (q+1)/2 + 1, t + q/2] is held.
__global__ void __launch_bounds__(kPqBlock) k_pq_dilate(PqGeom g, int q0, int q1, int q2,
                                                        const uint32_t* __restrict__ held, uint32_t* occ) {
  const int64_t t = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  if (t >= (int64_t)g.columns * g.wz) return;
  const int col = (int)(t / g.wz), wd = (int)(t % g.wz);
  const int x = col / g.dims[1], y = col % g.dims[1];
  const int x0 = max(0, x - (q0 + 1) / 2 + 1), x1 = min(g.dims[0] - 1, x + q0 / 2);
  const int y0 = max(0, y - (q1 + 1) / 2 + 1), y1 = min(g.dims[1] - 1, y + q1 / 2);
  uint32_t prev = 0, cur = 0, next = 0;
  for (int xx = x0; xx <= x1; ++xx)
    for (int yy = y0; yy <= y1; ++yy) {
      const uint32_t* hw = held + (int64_t)(xx * g.dims[1] + yy) * g.wz;
      cur |= hw[wd];
      if (wd > 0) prev |= hw[wd - 1];
      if (wd + 1 < g.wz) next |= hw[wd + 1];
    }
  // held bit z' marks z' + d, d in [-q2/2, (q2+1)/2 - 1]
  uint32_t o = cur;
  for (int d = 1; d <= (q2 + 1) / 2 - 1; ++d) o |= (cur << d) | (prev >> (32 - d));
  for (int e = 1; e <= q2 / 2; ++e) o |= (cur >> e) | (next << (32 - e));
  const int left = g.dims[2] - wd * 32;   // bits of this word inside the grid
  if (left < 32) o &= (1u << left) - 1u;
  occ[t] = o;
}

// ---------------------------------------------------------------- records
// One thread per listed point: a rank sort.  The point reads its column's keys
// (a few dozen, shared by the neighbouring lanes' points, all loads independent)
// and counts the smaller ones -- its place in the column's (z, id) order -- and
// those of its own voxel.  A voxel listing more than P points keeps the P of
// smallest res_pkey in ascending id: the others stay in place with id -1, which
// the walk skips.  Runs of voxels no floor-binned point holds (possible only for
// points the truncation moved) stay too; the walk tests the held bit first.
__global__ void __launch_bounds__(kPqBlock) k_pq_records(int64_t N, PqGeom g, int P, uint64_t seed,
                                                         const float* __restrict__ pers,
                                                         const int32_t* __restrict__ pcol,
                                                         const int32_t* __restrict__ pz,
                                                         const uint32_t* __restrict__ held,
                                                         const int32_t* __restrict__ col_off,
                                                         const uint64_t* __restrict__ keys, float4* rec,
                                                         int32_t* rec_z, pnr_pquery_stats* stats) {
  const int64_t i = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  int max_pts = 0;
  bool over = false;
  if (i < N && pcol[i] >= 0) {
    const int col = pcol[i], z = pz[i];
    const int base = col_off[col], n = col_off[col + 1] - base;
    const uint64_t mine = ((uint64_t)(uint32_t)z << 32) | (uint32_t)i;
    int rank = 0, cnt = 0, first = 1;
    for (int k = 0; k < n; ++k) {
      const uint64_t o = keys[base + k];
      rank += o < mine;
      const bool same = (int)(o >> 32) == z;
      cnt += same;
      first &= !(same && o < mine);
    }
    bool keep = true;
    if (cnt > P) {   // rank of this point's reservoir key among its voxel's
      const uint64_t pk = res_pkey(seed, (uint32_t)i);
      int r = 0;
      for (int k = 0; k < n; ++k) {
        const uint64_t o = keys[base + k];
        r += (int)(o >> 32) == z && res_pkey(seed, (uint32_t)o) < pk;
      }
      keep = r < P;
    }
    const Row3 p = reinterpret_cast<const Row3*>(pers)[i];
    rec[base + rank] = make_float4(p.x, p.y, p.z, __int_as_float(keep ? (int)i : -1));
    rec_z[base + rank] = z;
    if ((held[(int64_t)col * g.wz + (z >> 5)] >> (z & 31)) & 1u) {   // the voxel's statistics, by its first point
      max_pts = cnt;
      over = first && cnt > P;
    }
  }
  wave_count(&stats->n_voxels_over_p, over);
  const int mp = wave_max_i32(max_pts);
  if (mp && (threadIdx.x & 63) == 0) atomicMax(&stats->max_points_per_voxel, mp);
}

// One thread per column: the held voxels' count and its maximum.
__global__ void __launch_bounds__(kPqBlock) k_pq_colstats(PqGeom g, const uint32_t* __restrict__ held,
                                                          pnr_pquery_stats* stats) {
  const int col = blockIdx.x * kPqBlock + threadIdx.x;
  int n_held = 0;
  if (col < g.columns)
    for (int k = 0; k < g.wz; ++k) n_held += __popc(held[(int64_t)col * g.wz + k]);
  const int s = wave_sum_i32(n_held), mh = wave_max_i32(n_held);
  if (s && (threadIdx.x & 63) == 0) {
    atomicAdd(&stats->n_voxels_held, s);
    atomicMax(&stats->max_held_per_column, mh);
  }
}

// ---------------------------------------------------------------- select
__device__ __forceinline__ bool pixel_ok(int px, int py, const PqGeom& g) {
  return px >= 0 && px < g.w && py >= 0 && py < g.h;
}

__global__ void __launch_bounds__(kPqBlock) k_pq_select(PqGeom g, const int32_t* __restrict__ pixel_idx, int64_t R,
                                                        const uint32_t* __restrict__ occ, int32_t* hit,
                                                        int8_t* ray_mask, pnr_pquery_stats* stats) {
  const int64_t r = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  bool bad = false;
  if (r < R) {
    const int px = pixel_idx[r * 2], py = pixel_idx[r * 2 + 1];
    int far_id = -1;
    if (!pixel_ok(px, py, g)) {
      bad = true;
    } else {
      const uint32_t* ow = occ + (int64_t)((px / g.vscale[0]) * g.dims[1] + py / g.vscale[1]) * g.wz;
      for (int k = g.wz - 1; k >= 0; --k) {
        const uint32_t v = ow[k];
        if (v) {
          far_id = k * 32 + 31 - __clz(v);
          break;
        }
      }
    }
    const int m = far_id > 0;   // near_vox_full: a column that holds depth id 0 only is a miss
    hit[r] = m;
    ray_mask[r] = (int8_t)m;
  }
  wave_count(&stats->n_bad_pixels, bad);
}

// ------------------------------------------------------------------- knn
// The K ids and distances of a lane's sample: one column of the block's LDS
// arrays (query.hip KnnIds: a dynamic index is one ds access).
template <int KMAX>
struct PqIds {
  int32_t* p;
  float* q;
  __device__ __forceinline__ void set(int i, int32_t v, float d) {
    p[i * kPqKnnBlock] = v;
    q[i * kPqKnnBlock] = d;
  }
  __device__ __forceinline__ int32_t get(int i) const { return p[i * kPqKnnBlock]; }
  __device__ __forceinline__ float getd(int i) const { return q[i * kPqKnnBlock]; }
};

struct PqKnnArgs {
  PqGeom g;
  int SR, K, NN;
  int layers, zl_max;   // (kernel_size[0] + 1) / 2, (kernel_size[2] + 1) / 2 - 1
  float r2, d2;
  const int32_t* pixel_idx;
  int64_t R;
  const int32_t* hit;
  const int32_t* ray_off;
  const uint32_t* held;
  const uint32_t* occ;
  const int32_t* col_off;
  const int32_t* col_cnt;
  const float4* rec;
  const int32_t* rec_z;
  int32_t* pidx;     // [R, SR, K] rows in compact order
  float* loc;        // [R, SR, 3]
  int32_t* slot_z;   // [R, SR]
};

// The n-th (0-based) set bit of v; v has more than n bits set.
__device__ __forceinline__ int nth_bit(uint32_t v, int n) {
  for (int i = 0; i < n; ++i) v &= v - 1;
  return __ffs(v) - 1;
}

// One sample: the slot-th occupied depth id of pixel (px, py)'s column, its
// centre and (fz >= 0) the layered walk; the accepted ids are left in `ids`.
struct PqSample {
  int fz;             // depth id, -1: the column has no slot-th occupied id
  float cx, cy, cz;   // the centre
  int kid;            // neighbours kept (<= K)
};

template <int KMAX>
__device__ __forceinline__ PqSample pq_sample(const PqKnnArgs& a, int px, int py, int slot, PqIds<KMAX>& ids) {
  const PqGeom& g = a.g;
  const int fx = px / g.vscale[0], fy = py / g.vscale[1];
  const int col = fx * g.dims[1] + fy;
  // the slot-th occupied depth id of the column, or -1
  int fz = -1;
  {
    const uint32_t* ow = a.occ + (int64_t)col * g.wz;
    int left = slot;
    for (int k = 0; k < g.wz; ++k) {
      const uint32_t v = ow[k];
      const int c = __popc(v);
      if (left < c) {
        fz = k * 32 + nth_bit(v, left);
        break;
      }
      left -= c;
    }
  }
  // centres: float + int * float in fp32, the `+ 0.5` terms in double, one rounding to fp32
  const float cx = (float)((double)__fadd_rn(g.shift[0], __fmul_rn((float)fx, g.svs[0])) +
                           ((double)(px % g.vscale[0]) + 0.5) * (double)g.rvs[0]);
  const float cy = (float)((double)__fadd_rn(g.shift[1], __fmul_rn((float)fy, g.svs[1])) +
                           ((double)(py % g.vscale[1]) + 0.5) * (double)g.rvs[1]);
  const float cz = (float)((double)g.shift[2] + ((double)fz + 0.5) * (double)g.svs[2]);
  int kid = 0;
  if (fz >= 0) {
    int far_ind = 0;
    float far2 = 0.f;
    const float cxz = __fmul_rn(cx, cz), cyz = __fmul_rn(cy, cz);
    for (int layer = 0; layer < a.layers; ++layer) {
      const int zl = min(a.zl_max, layer);
      const int zlo = max(-fz, -zl), zhi = min(g.dims[2] - fz, zl + 1);
      for (int x = max(-fx, -layer); x < min(g.dims[0] - fx, layer + 1); ++x)
        for (int y = max(-fy, -layer); y < min(g.dims[1] - fy, layer + 1); ++y) {
          const bool ring = max(abs(x), abs(y)) == layer;
          const int c2 = (fx + x) * g.dims[1] + fy + y;
          const int base = a.col_off[c2], n = a.col_cnt[c2];
          const uint32_t* hw = a.held + (int64_t)c2 * g.wz;
          int at = 0;   // the column's records ascend in z: one pass serves the z loop
          for (int z = zlo; z < zhi && at < n; ++z) {
            if (!ring && (zl == layer ? abs(z) != zl : true)) continue;
            const int vz = fz + z;
            if (!((hw[vz >> 5] >> (vz & 31)) & 1u)) continue;
            while (at < n && a.rec_z[base + at] < vz) ++at;
            for (; at < n && a.rec_z[base + at] == vz; ++at) {
              const float4 v = a.rec[base + at];
              const int pid = __float_as_int(v.w);
              if (pid < 0) continue;   // cut by the P cap
              const float xv = a.NN < 2 ? __fsub_rn(v.x, cx) : __fsub_rn(__fmul_rn(v.x, v.z), cxz);
              const float yv = a.NN < 2 ? __fsub_rn(v.y, cy) : __fsub_rn(__fmul_rn(v.y, v.z), cyz);
              const float xy2 = __fadd_rn(__fmul_rn(xv, xv), __fmul_rn(yv, yv));
              const float zv = __fsub_rn(v.z, cz);
              const float z2 = __fmul_rn(zv, zv);
              const float d2 = __fadd_rn(xy2, z2);
              if (!((a.r2 == 0.f || xy2 <= a.r2) && (a.d2 == 0.f || z2 <= a.d2))) continue;
              if (kid < a.K) {
                ids.set(kid, pid, d2);
                if (d2 > far2) {
                  far2 = d2;
                  far_ind = kid;
                }
                ++kid;
              } else if (d2 < far2) {
                ids.set(far_ind, pid, d2);
                far2 = d2;
                for (int i = 0; i < a.K; ++i) {
                  const float b = ids.getd(i);
                  if (b > far2) {
                    far2 = b;
                    far_ind = i;
                  }
                }
              }
            }
          }
        }
    }
  }
  return PqSample{fz, cx, cy, cz, kid};
}

template <int KMAX>
__global__ void __launch_bounds__(kPqKnnBlock) k_pq_knn(PqKnnArgs a) {
  __shared__ int32_t ids_s[KMAX * kPqKnnBlock];
  __shared__ float dst_s[KMAX * kPqKnnBlock];
  const int64_t t = (int64_t)blockIdx.x * kPqKnnBlock + threadIdx.x;
  const int64_t r = t / a.SR;
  if (r >= a.R || !a.hit[r]) return;
  const int slot = (int)(t - r * a.SR);
  const int64_t row = (int64_t)a.ray_off[r] * a.SR + slot;
  PqIds<KMAX> ids{ids_s + threadIdx.x, dst_s + threadIdx.x};
  // inside the frame: the ray is a hit
  const PqSample s = pq_sample<KMAX>(a, a.pixel_idx[r * 2], a.pixel_idx[r * 2 + 1], slot, ids);
  reinterpret_cast<Row3*>(a.loc)[row] = Row3{s.cx, s.cy, s.cz};
  a.slot_z[row] = s.fz;
  int32_t* out = a.pidx + row * a.K;
  for (int i = 0; i < a.K; ++i) out[i] = i < s.kid ? ids.get(i) : -1;
}

// ------------------------------------------------- query buffers (pnr_pquery_bufs)
// One thread per ray: ray_hit = the querier's ray_mask, n_filled = the slots
// k_pq_knn would give a depth id (the column's occupied ids, at most SR).
__global__ void __launch_bounds__(kPqBlock) k_pq_columns(PqGeom g, int SR, const int32_t* __restrict__ pixel_idx,
                                                         int64_t R, const uint32_t* __restrict__ occ, int8_t* ray_hit,
                                                         int32_t* n_filled, int32_t* counts) {
  const int64_t r = (int64_t)blockIdx.x * kPqBlock + threadIdx.x;
  bool hit = false;
  if (r < R) {
    const int px = pixel_idx[r * 2], py = pixel_idx[r * 2 + 1];
    int far_id = -1, n = 0;
    if (pixel_ok(px, py, g)) {
      const uint32_t* ow = occ + (int64_t)((px / g.vscale[0]) * g.dims[1] + py / g.vscale[1]) * g.wz;
      for (int k = 0; k < g.wz; ++k) {
        const uint32_t v = ow[k];
        n += __popc(v);
        if (v) far_id = k * 32 + 31 - __clz(v);
      }
    }
    hit = far_id > 0;   // near_vox_full: a column that holds depth id 0 only is a miss
    ray_hit[r] = (int8_t)hit;
    n_filled[r] = hit ? min(n, SR) : 0;
  }
  wave_count(counts + 2, hit);   // R_hit
}

struct PqFillArgs {
  PqKnnArgs k;   // pidx / loc / slot_z / hit unused
  const float* campos;   // [3]
  const float* camrot;   // [3,3] camrotc2w
  const int32_t* n_filled;
  int32_t* fill_rs;
  uint16_t* slot_d;
  int32_t* pidx;        // [S_filled, K]
  float* sample_p;      // [S_filled, 3]
  float* sample_w;
  float* sample_dir;
  int32_t* vflag;
  int32_t* ray_vcnt;
  int32_t* counts;
  int vec_pidx;         // pidx rows are 16-byte aligned (K % 4 == 0, aligned base)
};

// One thread per (ray, slot): a slot below n_filled has a depth id, so every
// thread that passes the test walks (pq_sample: k_pq_knn's own code) and writes
// filled sample ray_off[r] + slot.  pers2w (query_point_indices.py:104-116) in
// its fp32 order: xyz_c = (cx cz, cy cz, cz), shift_i = sum_j xyz_c[j] camrot[i][j],
// dir = shift / (|shift| + 1e-7), w = shift + campos.
__global__ void __launch_bounds__(kPqKnnBlock) k_pq_fill(PqFillArgs f) {
  __shared__ int32_t ids_s[8 * kPqKnnBlock];
  __shared__ float dst_s[8 * kPqKnnBlock];
  const PqKnnArgs& a = f.k;
  const int64_t t = (int64_t)blockIdx.x * kPqKnnBlock + threadIdx.x;
  const int64_t r = t / a.SR;
  const int slot = (int)(t - r * a.SR);
  int pairs = 0;
  if (r < a.R && slot < f.n_filled[r]) {
    const int64_t i = (int64_t)a.ray_off[r] + slot;
    PqIds<8> ids{ids_s + threadIdx.x, dst_s + threadIdx.x};
    const PqSample s = pq_sample<8>(a, a.pixel_idx[r * 2], a.pixel_idx[r * 2 + 1], slot, ids);
    f.fill_rs[i] = (int32_t)(r * a.SR + slot);
    f.slot_d[i] = (uint16_t)s.fz;
    if (f.vec_pidx) {
      int4* o4 = reinterpret_cast<int4*>(f.pidx + i * a.K);
      for (int k = 0; k < a.K; k += 4)
        o4[k >> 2] = make_int4(k < s.kid ? ids.get(k) : -1, k + 1 < s.kid ? ids.get(k + 1) : -1,
                               k + 2 < s.kid ? ids.get(k + 2) : -1, k + 3 < s.kid ? ids.get(k + 3) : -1);
    } else {
      for (int k = 0; k < a.K; ++k) f.pidx[i * a.K + k] = k < s.kid ? ids.get(k) : -1;
    }
    reinterpret_cast<Row3*>(f.sample_p)[i] = Row3{s.cx, s.cy, s.cz};
    const float xc[3] = {__fmul_rn(s.cx, s.cz), __fmul_rn(s.cy, s.cz), s.cz};
    float sh[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
      sh[m] = __fadd_rn(__fadd_rn(__fmul_rn(xc[0], f.camrot[m * 3]), __fmul_rn(xc[1], f.camrot[m * 3 + 1])),
                        __fmul_rn(xc[2], f.camrot[m * 3 + 2]));
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(sh[0], sh[0]), __fmul_rn(sh[1], sh[1])), __fmul_rn(sh[2], sh[2]));
    const float den = __fadd_rn(__fsqrt_rn(n2), 1e-7f);
    reinterpret_cast<Row3*>(f.sample_dir)[i] =
        Row3{__fdiv_rn(sh[0], den), __fdiv_rn(sh[1], den), __fdiv_rn(sh[2], den)};
    reinterpret_cast<Row3*>(f.sample_w)[i] =
        Row3{__fadd_rn(sh[0], f.campos[0]), __fadd_rn(sh[1], f.campos[1]), __fadd_rn(sh[2], f.campos[2])};
    f.vflag[i] = s.kid > 0;
    if (s.kid > 0) atomicAdd(f.ray_vcnt + r, 1);
    pairs = s.kid;
  }
  pairs = wave_sum_i32(pairs);
  if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(f.counts + 4, pairs);
}

// --------------------------------------------------------------- compact
__global__ void __launch_bounds__(kPqBlock) k_pq_copy(const int32_t* __restrict__ src_i, int32_t* dst_i, int64_t n_i,
                                                      const float* __restrict__ src_f, float* dst_f, int64_t n_f) {
  for (int64_t i = (int64_t)blockIdx.x * kPqBlock + threadIdx.x; i < n_i + n_f; i += (int64_t)gridDim.x * kPqBlock) {
    if (i < n_i)
      dst_i[i] = src_i[i];
    else
      dst_f[i - n_i] = src_f[i - n_i];
  }
}

inline int check_pq(const char* who, const pnr_pquery_params* q, PqGeom* g) {
  PNR_CHECK_ARG(q, "%s: null params", who);
  for (int k = 0; k < 3; ++k) {
    PNR_CHECK_ARG(q->dims[k] >= 1 && q->vscale[k] >= 1, "%s: dims[%d]=%d vscale[%d]=%d (>= 1)", who, k, q->dims[k], k,
                  q->vscale[k]);
    PNR_CHECK_ARG(q->scaled_vsize[k] > 0.f && q->scaled_vsize[k] < __builtin_inff() && q->ray_vsize[k] > 0.f &&
                      q->ray_vsize[k] < __builtin_inff(),
                  "%s: voxel size of axis %d is not positive and finite", who, k);
    PNR_CHECK_ARG(q->kernel_size[k] >= 1 && q->kernel_size[k] <= kPqMaxSize && q->query_size[k] >= 1 &&
                      q->query_size[k] <= kPqMaxSize,
                  "%s: kernel_size[%d]=%d query_size[%d]=%d (1 .. %d)", who, k, q->kernel_size[k], k, q->query_size[k],
                  kPqMaxSize);
  }
  PNR_CHECK_ARG(q->w >= 1 && q->h >= 1, "%s: w=%d h=%d (>= 1)", who, q->w, q->h);
  PNR_CHECK_ARG((int64_t)q->dims[0] * q->vscale[0] >= q->w && (int64_t)q->dims[1] * q->vscale[1] >= q->h,
                "%s: dims * vscale = %lld x %lld does not cover the %d x %d frame", who,
                (long long)q->dims[0] * q->vscale[0], (long long)q->dims[1] * q->vscale[1], q->w, q->h);
  const int64_t columns = (int64_t)q->dims[0] * q->dims[1];
  const int wz = (q->dims[2] + 31) / 32;
  PNR_CHECK_ARG(columns * wz < (int64_t)1 << 30, "%s: %lld columns of %d depth words: too many", who,
                (long long)columns, wz);
  PNR_CHECK_ARG(q->SR >= 1 && q->K >= 1 && q->K <= 32 && q->P >= 1, "%s: SR=%d K=%d P=%d (SR, P >= 1; K in 1..32)", who,
                q->SR, q->K, q->P);
  PNR_CHECK_ARG(q->NN >= 1, "%s: NN=%d: the random query (NN = 0) is not supported", who, q->NN);
  PNR_CHECK_ARG(q->radius_limit2 >= 0.f && q->depth_limit2 >= 0.f, "%s: negative limit", who);
  // every voxel a walk can visit must lie inside the block marked round the sample's own voxel
  const int hx = (q->kernel_size[0] + 1) / 2 - 1;
  const int hz = hx < (q->kernel_size[2] + 1) / 2 - 1 ? hx : (q->kernel_size[2] + 1) / 2 - 1;
  PNR_CHECK_ARG(hx <= (q->query_size[0] + 1) / 2 - 1 && hx <= (q->query_size[1] + 1) / 2 - 1 &&
                    hz <= (q->query_size[2] + 1) / 2 - 1,
                "%s: kernel_size (%d, %d, %d) is wider than query_size (%d, %d, %d): a ray's neighbours would depend "
                "on the other rays of the batch",
                who, q->kernel_size[0], q->kernel_size[1], q->kernel_size[2], q->query_size[0], q->query_size[1],
                q->query_size[2]);
  for (int k = 0; k < 3; ++k) {
    g->shift[k] = q->shift[k], g->svs[k] = q->scaled_vsize[k], g->rvs[k] = q->ray_vsize[k];
    g->dims[k] = q->dims[k], g->vscale[k] = q->vscale[k];
  }
  g->w = q->w, g->h = q->h, g->wz = wz, g->columns = (int)columns;
  return PNR_OK;
}

inline int check_pq_sizes(const char* who, int64_t N, int64_t R, int32_t SR, int32_t K) {
  PNR_CHECK_ARG(N >= 0 && N < (int64_t)1 << 31, "%s: N=%lld outside [0, 2^31)", who, (long long)N);
  PNR_CHECK_ARG(R >= 0 && SR >= 1 && K >= 1 && R * SR < (int64_t)1 << 31, "%s: R=%lld SR=%d (R * SR below 2^31)", who,
                (long long)R, SR);
  return PNR_OK;
}

// The per-camera part: bin, scan, scatter, dilate, column statistics, records.
// Its tables (held, occ, col_cnt, col_off, rec, rec_z) sit in front of the
// per-ray parts of the layout, so their places do not depend on R.
inline int pq_build(const pnr_pquery_params& q, const PqGeom& g, const float* xyz_pers, int64_t N, const PqScratch& s,
                    void* scratch, pnr_pquery_stats* stats, hipStream_t st) {
  PNR_HIP(hipMemsetAsync(scratch, 0, s.zero_bytes, st));
  PNR_HIP(hipMemsetAsync(stats, 0, sizeof(pnr_pquery_stats), st));
  if (N > 0) {
    hipLaunchKernelGGL(k_pq_bin, dim3((unsigned)cdiv(N, kPqBlock)), dim3(kPqBlock), 0, st, xyz_pers, N, g, s.held,
                       s.col_cnt, s.pcol, s.pz, stats);
    PNR_LAUNCH_CHECK();
  }
  if (int rc = exclusive_scan(s.col_cnt, g.columns, nullptr, s.col_off, (int64_t)g.columns + 1, nullptr, s.scan,
                              s.scan_bytes, st))
    return rc;
  if (N > 0) {
    hipLaunchKernelGGL(k_pq_scatter, dim3((unsigned)cdiv(N, kPqBlock)), dim3(kPqBlock), 0, st, N, s.pcol, s.pz,
                       s.col_off, s.col_cur, s.keys);
    PNR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pq_dilate, dim3((unsigned)cdiv((int64_t)g.columns * g.wz, kPqBlock)), dim3(kPqBlock), 0, st, g,
                     q.query_size[0], q.query_size[1], q.query_size[2], s.held, s.occ);
  PNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pq_colstats, dim3((unsigned)cdiv(g.columns, kPqBlock)), dim3(kPqBlock), 0, st, g, s.held, stats);
  PNR_LAUNCH_CHECK();
  if (N > 0) {
    hipLaunchKernelGGL(k_pq_records, dim3((unsigned)cdiv(N, kPqBlock)), dim3(kPqBlock), 0, st, N, g, q.P,
                       (uint64_t)q.grid_seed, xyz_pers, s.pcol, s.pz, s.held, s.col_off, s.keys, s.rec, s.rec_z,
                       stats);
    PNR_LAUNCH_CHECK();
  }
  return PNR_OK;
}

// What the walk reads of a build, and the call's rays.
inline PqKnnArgs pq_knn_args(const pnr_pquery_params& q, const PqGeom& g, const PqScratch& s, const int32_t* pixel_idx,
                             int64_t R) {
  PqKnnArgs a = {};
  a.g = g, a.SR = q.SR, a.K = q.K, a.NN = q.NN;
  a.layers = (q.kernel_size[0] + 1) / 2, a.zl_max = (q.kernel_size[2] + 1) / 2 - 1;
  a.r2 = q.radius_limit2, a.d2 = q.depth_limit2;
  a.pixel_idx = pixel_idx, a.R = R, a.held = s.held, a.occ = s.occ;
  a.col_off = s.col_off, a.col_cnt = s.col_cnt, a.rec = s.rec, a.rec_z = s.rec_z;
  return a;
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_pquery_scratch_bytes(int64_t N, int64_t R, int32_t SR, const int32_t* dims, size_t* out) {
  PNR_CHECK_ARG(out && dims, "pquery_scratch_bytes: null pointer");
  if (int rc = check_pq_sizes("pquery_scratch_bytes", N, R, SR, 1)) return rc;
  PNR_CHECK_ARG(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "pquery_scratch_bytes: dims (%d, %d, %d)", dims[0],
                dims[1], dims[2]);
  const int64_t columns = (int64_t)dims[0] * dims[1];
  const int wz = (dims[2] + 31) / 32;
  PNR_CHECK_ARG(columns * wz < (int64_t)1 << 30, "pquery_scratch_bytes: %lld columns of %d depth words: too many",
                (long long)columns, wz);
  *out = pq_layout(nullptr, N, R, columns, wz).total;
  return PNR_OK;
}

extern "C" int pnr_pquery(const pnr_pquery_params* params_host, const float* xyz_pers, int64_t N,
                          const int32_t* pixel_idx, int64_t R, int32_t* sample_pidx, float* sample_loc,
                          int32_t* slot_z, int8_t* ray_mask, int32_t* counts, pnr_pquery_stats* stats, void* scratch,
                          size_t scratch_bytes, void* stream) {
  PqGeom g;
  if (int rc = check_pq("pquery", params_host, &g)) return rc;
  const pnr_pquery_params& q = *params_host;
  if (int rc = check_pq_sizes("pquery", N, R, q.SR, q.K)) return rc;
  PNR_CHECK_ARG(counts && stats && scratch, "pquery: null pointer");
  PNR_CHECK_ARG(N == 0 || xyz_pers, "pquery: null points");
  PNR_CHECK_ARG(R == 0 || (pixel_idx && sample_pidx && sample_loc && slot_z && ray_mask), "pquery: null ray buffer");
  const PqScratch s = pq_layout(scratch, N, R, g.columns, g.wz);
  PNR_CHECK_ARG(scratch_bytes >= s.total, "pquery: scratch too small (%zu < %zu)", scratch_bytes, s.total);
  hipStream_t st = as_stream(stream);
  if (int rc = pq_build(q, g, xyz_pers, N, s, scratch, stats, st)) return rc;
  if (R > 0) {
    hipLaunchKernelGGL(k_pq_select, dim3((unsigned)cdiv(R, kPqBlock)), dim3(kPqBlock), 0, st, g, pixel_idx, R, s.occ,
                       s.hit, ray_mask, stats);
    PNR_LAUNCH_CHECK();
  }
  if (int rc = exclusive_scan(s.hit, R, nullptr, s.ray_off, R + 1, counts, s.scan, s.scan_bytes, st)) return rc;
  if (R > 0) {
    PqKnnArgs a = pq_knn_args(q, g, s, pixel_idx, R);
    a.hit = s.hit, a.ray_off = s.ray_off;
    a.pidx = sample_pidx, a.loc = sample_loc, a.slot_z = slot_z;
    const dim3 grid((unsigned)cdiv(R * q.SR, kPqKnnBlock)), block(kPqKnnBlock);
    if (q.K <= 8)
      hipLaunchKernelGGL(k_pq_knn<8>, grid, block, 0, st, a);
    else if (q.K <= 16)
      hipLaunchKernelGGL(k_pq_knn<16>, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(k_pq_knn<32>, grid, block, 0, st, a);
    PNR_LAUNCH_CHECK();
  }
  return PNR_OK;
}

// The build alone, into scratch of pnr_pquery_scratch_bytes(N, 0, SR, dims): what
// every pnr_pquery_bufs call of one camera and cloud reads.
extern "C" int pnr_pquery_build(const pnr_pquery_params* params_host, const float* xyz_pers, int64_t N,
                                pnr_pquery_stats* stats, void* scratch, size_t scratch_bytes, void* stream) {
  PqGeom g;
  if (int rc = check_pq("pquery_build", params_host, &g)) return rc;
  const pnr_pquery_params& q = *params_host;
  if (int rc = check_pq_sizes("pquery_build", N, 0, q.SR, q.K)) return rc;
  PNR_CHECK_ARG(stats && scratch, "pquery_build: null pointer");
  PNR_CHECK_ARG(N == 0 || xyz_pers, "pquery_build: null points");
  const PqScratch s = pq_layout(scratch, N, 0, g.columns, g.wz);
  PNR_CHECK_ARG(scratch_bytes >= s.total, "pquery_build: scratch too small (%zu < %zu)", scratch_bytes, s.total);
  return pq_build(q, g, xyz_pers, N, s, scratch, stats, as_stream(stream));
}

extern "C" int pnr_pquery_bufs(const pnr_pquery_params* params_host, int64_t N, const int32_t* pixel_idx, int64_t R,
                               const float* campos, const float* camrot, pnr_query_bufs* b, int8_t* ray_hit,
                               float* sample_dir, const void* build, size_t build_bytes, void* stream) {
  PqGeom g;
  if (int rc = check_pq("pquery_bufs", params_host, &g)) return rc;
  const pnr_pquery_params& q = *params_host;
  if (int rc = check_pq_sizes("pquery_bufs", N, R, q.SR, q.K)) return rc;
  PNR_CHECK_ARG(q.K <= 8, "pquery_bufs: K=%d (1 .. 8, the aggregate's limit)", q.K);
  PNR_CHECK_ARG(q.dims[2] <= 65535, "pquery_bufs: dims[2]=%d depth ids do not fit slot_d (<= 65535)", q.dims[2]);
  PNR_CHECK_ARG(b && build && campos && camrot, "pquery_bufs: null pointer");
  PNR_CHECK_ARG(b->n_filled && b->slot_d && b->ray_off && b->fill_rs && b->pidx && b->valid_off && b->valid_list &&
                    b->vflag && b->ray_vcnt && b->ray_row && b->sample_w && b->sample_p && b->counts && b->scratch,
                "pquery_bufs: null buffer");
  PNR_CHECK_ARG(R == 0 || (pixel_idx && ray_hit && sample_dir), "pquery_bufs: null ray buffer");
  const PqScratch s = pq_layout(const_cast<void*>(build), N, 0, g.columns, g.wz);
  PNR_CHECK_ARG(build_bytes >= s.total, "pquery_bufs: build scratch too small (%zu < %zu)", build_bytes, s.total);
  const int64_t RS = R * q.SR;
  PNR_CHECK_ARG(b->scratch_bytes >= scan_scratch_bytes(RS + 1), "pquery_bufs: scan scratch too small");
  hipStream_t st = as_stream(stream);
  PNR_HIP(hipMemsetAsync(b->counts, 0, 8 * sizeof(int32_t), st));
  PNR_HIP(hipMemsetAsync(b->ray_vcnt, 0, (size_t)(R > 0 ? R : 1) * sizeof(int32_t), st));
  if (R == 0) {
    PNR_HIP(hipMemsetAsync(b->ray_off, 0, sizeof(int32_t), st));
    PNR_HIP(hipMemsetAsync(b->ray_row, 0, sizeof(int32_t), st));
    PNR_HIP(hipMemsetAsync(b->valid_off, 0, sizeof(int32_t), st));
    return PNR_OK;
  }
  hipLaunchKernelGGL(k_pq_columns, dim3((unsigned)cdiv(R, kPqBlock)), dim3(kPqBlock), 0, st, g, q.SR, pixel_idx, R,
                     s.occ, ray_hit, b->n_filled, b->counts);
  PNR_LAUNCH_CHECK();
  if (int rc = exclusive_scan(b->n_filled, R, nullptr, b->ray_off, R + 1, b->counts + 0, b->scratch, b->scratch_bytes,
                              st))
    return rc;
  PqFillArgs f = {};
  f.k = pq_knn_args(q, g, s, pixel_idx, R);
  f.k.ray_off = b->ray_off;
  f.campos = campos, f.camrot = camrot, f.n_filled = b->n_filled, f.fill_rs = b->fill_rs, f.slot_d = b->slot_d;
  f.pidx = b->pidx, f.sample_p = b->sample_p, f.sample_w = b->sample_w, f.sample_dir = sample_dir;
  f.vflag = b->vflag, f.ray_vcnt = b->ray_vcnt, f.counts = b->counts;
  f.vec_pidx = q.K % 4 == 0 && ((uintptr_t)b->pidx & 15) == 0;
  hipLaunchKernelGGL(k_pq_fill, dim3((unsigned)cdiv(RS, kPqKnnBlock)), dim3(kPqKnnBlock), 0, st, f);
  PNR_LAUNCH_CHECK();
  if (int rc = exclusive_scan(b->vflag, RS, b->counts + 0, b->valid_off, RS + 1, b->counts + 1, b->scratch,
                              b->scratch_bytes, st, 0, nullptr, b->valid_list))
    return rc;
  return exclusive_scan(b->ray_vcnt, R, nullptr, b->ray_row, R + 1, b->counts + 3, b->scratch, b->scratch_bytes, st,
                        /*as_flag=*/1);
}

extern "C" int pnr_pquery_compact(const int32_t* pidx_rows, const float* loc_rows, int64_t R, int32_t SR, int32_t K,
                                  int64_t R_hit, int32_t* sample_pidx, float* sample_loc, void* stream) {
  if (int rc = check_pq_sizes("pquery_compact", 0, R, SR, K)) return rc;
  PNR_CHECK_ARG(R_hit >= 0 && R_hit <= R, "pquery_compact: R'=%lld outside [0, R=%lld]", (long long)R_hit,
                (long long)R);
  if (R_hit == 0) return PNR_OK;
  PNR_CHECK_ARG(pidx_rows && loc_rows && sample_pidx && sample_loc, "pquery_compact: null pointer");
  const int64_t n_i = R_hit * SR * K, n_f = R_hit * SR * 3;
  hipLaunchKernelGGL(k_pq_copy, dim3(grid_for(n_i + n_f, kPqBlock)), dim3(kPqBlock), 0, as_stream(stream), pidx_rows,
                     sample_pidx, n_i, loc_rows, sample_loc, n_f);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
