// Shared host/device helpers for libpnr.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/pnr.h"

namespace pnr {

// ------------------------------------------------------------ error plumbing
void set_error(const char* fmt, ...);

#define PNR_CHECK_ARG(cond, ...)          \
  do {                                    \
    if (!(cond)) {                        \
      ::pnr::set_error(__VA_ARGS__);      \
      return PNR_EINVAL;                  \
    }                                     \
  } while (0)

#define PNR_HIP(call)                                                         \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      ::pnr::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call,           \
                       hipGetErrorString(e_));                                \
      return PNR_EHIP;                                                        \
    }                                                                         \
  } while (0)

#define PNR_LAUNCH_CHECK() PNR_HIP(hipGetLastError())

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Persistent-grid launch size for grid-stride kernels: enough workgroups to
// fill 256 CUs several times over, never more than the work needs.
inline unsigned grid_for(int64_t items, int block, int max_blocks = 256 * 8) {
  int64_t g = cdiv(items, block);
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (unsigned)g;
}

// Device-wide exclusive scan (scan.hip).
int64_t scan_blocks(int64_t n);
size_t scan_scratch_bytes(int64_t n);
// out_cap: int32 entries the caller allocated at out; the scan writes out[0 .. n]
// (n + 1 entries: the grand total lands at out[n_eff]), checked here.
int exclusive_scan(const int32_t* in, int64_t n, const int32_t* n_dev, int32_t* out, int64_t out_cap,
                   int32_t* total_dev, void* scratch, size_t scratch_bytes, hipStream_t st,
                   int as_flag = 0,   // as_flag: scan (in[i] != 0) instead of in[i]
                   const int32_t* run_if = nullptr,   // device flag: 0 = leave out untouched
                   int32_t* list = nullptr);          // optional stream compaction: list[out[i]] = i for in[i] != 0

// --------------------------------------------------------- device helpers
// floor((p - shift) / vs) exactly as the reference kernels compute it in fp32
// (qpiw.py:265-267, 406-408, 471-473): one rounded subtraction, one correctly
// rounded division, floor, truncating cast.
__device__ __forceinline__ int vox_coord(float p, float shift, float vs) {
  return (int)floorf(__fdiv_rn(__fsub_rn(p, shift), vs));
}

// vox_coord's value without the IEEE division on almost every call: t = x * inv
// (inv = RN(1 / vs)) is within |e| 2^-22 of e = x / vs and RN(e) within |e| 2^-24,
// so when t is farther than |t| 2^-20 from every integer, floor(t) is
// floor(RN(e)); otherwise (an integer within reach, x = 0) the exact division.
__device__ __forceinline__ int vox_coord_fast(float p, float shift, float vs, float inv) {
  const float x = __fsub_rn(p, shift);
  const float t = __fmul_rn(x, inv);
  const float f = floorf(t);
  const float m = __fmaf_rn(fabsf(t), 0x1p-20f, 0x1p-100f);
  if (__fsub_rn(t, f) > m && __fsub_rn(__fadd_rn(f, 1.0f), t) > m) return (int)f;
  return (int)floorf(__fdiv_rn(x, vs));
}

// raypos = campos + raydir * t  (diff_ray_marching.py:387: mul, then add).
__device__ __forceinline__ float ray_at(float c, float d, float t) {
  return __fadd_rn(c, __fmul_rn(d, t));
}

// Camera-space coordinates, xyz_c_j = sum_i (p_i - c_i) * R[i][j] with the
// reference's summation order (qpiw.py:104-105, neural_points.py:687-693).
__device__ __forceinline__ void world_to_cam(const float p[3], const float c[3],
                                             const float R[9], float out[3]) {
  float s0 = __fsub_rn(p[0], c[0]);
  float s1 = __fsub_rn(p[1], c[1]);
  float s2 = __fsub_rn(p[2], c[2]);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float a = __fmul_rn(s0, R[0 * 3 + j]);
    float b = __fmul_rn(s1, R[1 * 3 + j]);
    float d = __fmul_rn(s2, R[2 * 3 + j]);
    out[j] = __fadd_rn(__fadd_rn(a, b), d);
  }
}

// (x/z, y/z, z)
__device__ __forceinline__ void world_to_pers(const float p[3], const float c[3],
                                              const float R[9], float out[3]) {
  float xc[3];
  world_to_cam(p, c, R, xc);
  out[0] = __fdiv_rn(xc[0], xc[2]);
  out[1] = __fdiv_rn(xc[1], xc[2]);
  out[2] = xc[2];
}

// One row of the device camera table (rays.py camera_table): camrotc2w 9,
// campos 3, fx, fy, cx, cy.
constexpr int kCamRow = 16;

struct __attribute__((packed, aligned(4))) Row3 {
  float x, y, z;
};
struct __attribute__((packed, aligned(4))) Row2 {
  float x, y;
};

// get_dtu_raydir of one pixel (data/data_utils.py:55-69):
// x = ((px + 0.5f) - cx) / fx in three correctly rounded fp32 operations, the
// rotation in fp64 on the widened fp32 entries, (x R[i][0] + y R[i][1]) +
// R[i][2] left to right without FMA, one rounding to fp32.
__device__ __forceinline__ Row3 pixel_dir(float px, float py, const float* __restrict__ cam, int dir_norm) {
  const float x = __fdiv_rn(__fsub_rn(__fadd_rn(px, 0.5f), cam[14]), cam[12]);
  const float y = __fdiv_rn(__fsub_rn(__fadd_rn(py, 0.5f), cam[15]), cam[13]);
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = __dmul_rn((double)x, (double)cam[i * 3]);
    const double b = __dmul_rn((double)y, (double)cam[i * 3 + 1]);
    d[i] = __dadd_rn(__dadd_rn(a, b), (double)cam[i * 3 + 2]);
  }
  if (dir_norm) {   // dirs / (norm + 1e-5), data_utils.py:64-66
    const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2]));
    const double den = __dadd_rn(__dsqrt_rn(n2), 1e-5);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = __ddiv_rn(d[i], den);
  }
  return Row3{(float)d[0], (float)d[1], (float)d[2]};
}

// (u, v) = (fx cx / cz + cx0, fy cy / cz + cy0): the continuous pixel position
// of a camera-space point; pixel (i, j) covers [i, i+1) x [j, j+1).
__device__ __forceinline__ void project(const float xc[3], const float* cam, float* u, float* v) {
  *u = __fadd_rn(__fdiv_rn(__fmul_rn(cam[12], xc[0]), xc[2]), cam[14]);
  *v = __fadd_rn(__fdiv_rn(__fmul_rn(cam[13], xc[1]), xc[2]), cam[15]);
}

__device__ __forceinline__ bool in_image(float u, float v, int W, int H) {   // false for NaN
  return u >= 0.f && u < (float)W && v >= 0.f && v < (float)H;
}

// Bilinear blend of four taps with weights (wx, wy) towards c01 / c10.
__device__ __forceinline__ float lerp2(float c00, float c01, float c10, float c11, float wx, float wy) {
  const float ux = __fsub_rn(1.f, wx), uy = __fsub_rn(1.f, wy);
  const float top = __fadd_rn(__fmul_rn(ux, c00), __fmul_rn(wx, c01));
  const float bot = __fadd_rn(__fmul_rn(ux, c10), __fmul_rn(wx, c11));
  return __fadd_rn(__fmul_rn(uy, top), __fmul_rn(wy, bot));
}

// Seeded reservoir of the grid build (max_o / P overflow, qpiw.py:289-298,
// 377-384): a uniform random subset chosen by the smallest keys
// hash32(seed, id) << 32 | id (oracle/query_ref.c states the same keys).
constexpr uint64_t kPtSalt = 0x632BE59BD9B4E019ull;
__host__ __device__ inline uint32_t res_hash32(uint64_t seed, uint32_t id) {
  uint64_t z = seed ^ ((uint64_t)id * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}
__host__ __device__ inline uint64_t res_vkey(uint64_t seed, uint32_t id) {
  return ((uint64_t)res_hash32(seed, id) << 32) | id;
}
__host__ __device__ inline uint64_t res_pkey(uint64_t seed, uint32_t id) {
  return ((uint64_t)res_hash32(seed + kPtSalt, id) << 32) | id;
}
__host__ __device__ inline uint32_t res_pkey_hash(uint64_t seed, uint32_t id) {   // res_pkey's high half
  return res_hash32(seed + kPtSalt, id);
}

// Sum over the 64 lanes of a wave.
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace pnr
