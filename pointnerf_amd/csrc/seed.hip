// Neural-point seeding from a raw cloud and posed images: the
// geometric part of the reference's initialisation, run/train_ft.py:678-740 --
// the `ranges` box, mvs_utils.alpha_masking (the visual-hull carve against
// every view's alpha mask, models/mvs/mvs_utils.py:573-607), nearest_view
// (train_ft.py:42-51) and the per-view colour / direction lookup of
// query_embedding(pointdir_w=True).  Three kernels, one thread per point or
// pixel: k_alpha_bits thresholds the masks once into bit planes, k_seed_mask
// votes every point against every view, k_seed_view picks each survivor's
// view and samples it.  Both point kernels stage the camera table through LDS
// in tiles; every lane reads the same camera, an LDS broadcast.
//
// Arithmetic: fp32, one rounding per operation, in the order written here
// (this file is built with -ffp-contract=off); tests/seed_ref.py restates it
// in fp64.
#include "pnr_common.h"

namespace pnr {

constexpr int kSeedBlock = 256;
constexpr int kSeedTile = PNR_SEED_CAM_TILE;

// ------------------------------------------------------------- bit planes
// bits[(f H + y) pitch + x / 32] bit (x % 32) = alpha[f, y, x] > 0.1 (uint8
// masks are read as / 255).  One wave per 64 pixels of a row: the ballot is the
// two words.  Padding bits past W are 0.
struct AlphaBitsArgs {
  const void* alphas;
  uint32_t* bits;
  int64_t rows;   // F * H
  int W, pitch, u8;
};

__global__ void __launch_bounds__(kSeedBlock) k_alpha_bits(AlphaBitsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t chunks = cdiv(a.W, 64);
  const int64_t items = a.rows * chunks;
  const int64_t waves = (int64_t)gridDim.x * (kSeedBlock / 64);
  for (int64_t it = (int64_t)blockIdx.x * (kSeedBlock / 64) + (threadIdx.x >> 6); it < items; it += waves) {
    const int64_t row = it / chunks;
    const int ch = (int)(it % chunks);
    const int x = ch * 64 + lane;
    bool on = false;
    if (x < a.W) {
      const int64_t at = row * a.W + x;
      const float v = a.u8 ? __fdiv_rn((float)static_cast<const uint8_t*>(a.alphas)[at], 255.0f)
                           : static_cast<const float*>(a.alphas)[at];
      on = v > 0.1f;
    }
    const uint64_t b = __ballot(on);
    const int w = ch * 2 + lane;
    if (lane < 2 && w < a.pitch) a.bits[row * a.pitch + w] = (uint32_t)(b >> (32 * lane));
  }
}

// ------------------------------------------------------------------- mask
struct SeedMaskArgs {
  const float* xyz;       // [N,3]
  const float* cams;      // [F,16]
  const uint32_t* bits;   // bit planes or nullptr: no hull vote
  int64_t N;
  int F, H, W, pitch;
  int use_ranges, use_nf, inall, views;   // views: the view loop runs (bits or near_far)
  float lo[3], hi[3];
  float nf_lo, nf_hi;     // near - 1, far
  int32_t* keep;          // [N] 1 = survivor
};

__global__ void __launch_bounds__(kSeedBlock) k_seed_mask(SeedMaskArgs a) {
  __shared__ float cam_s[kSeedTile * kCamRow];
  const int64_t n = (int64_t)blockIdx.x * kSeedBlock + threadIdx.x;
  bool alive = n < a.N;
  float p[3] = {0.f, 0.f, 0.f};
  if (alive) {
    const Row3 r = reinterpret_cast<const Row3*>(a.xyz)[n];
    p[0] = r.x, p[1] = r.y, p[2] = r.z;
    if (a.use_ranges)
      alive = p[0] >= a.lo[0] && p[0] <= a.hi[0] && p[1] >= a.lo[1] && p[1] <= a.hi[1] && p[2] >= a.lo[2] &&
              p[2] <= a.hi[2];
  }
  if (a.views) {
    for (int f0 = 0; f0 < a.F; f0 += kSeedTile) {
      // the barrier that frees the previous tile also tells whether anyone is left
      if (!__syncthreads_or(alive)) break;
      const int cnt = min(kSeedTile, a.F - f0);
      for (int i = threadIdx.x; i < cnt * kCamRow; i += kSeedBlock) cam_s[i] = a.cams[(int64_t)f0 * kCamRow + i];
      __syncthreads();
      if (__ballot(alive) == 0) continue;   // this wave is carved: it only keeps the barriers
      for (int j = 0; j < cnt; ++j) {
        if (alive) {
          const float* cam = cam_s + j * kCamRow;
          float xc[3];
          world_to_cam(p, cam + 9, cam, xc);
          const float cz = xc[2];
          bool ok = true;
          if (a.bits) {
            float u, v;
            project(xc, cam, &u, &v);
            const bool inside = cz > 0.f && in_image(u, v, a.W, a.H);
            if (inside || (a.inall && cz > 0.f)) {   // outside and inall_img: the border pixel
              const int x = (int)fminf(fmaxf(floorf(u), 0.f), (float)(a.W - 1));
              const int y = (int)fminf(fmaxf(floorf(v), 0.f), (float)(a.H - 1));
              const uint32_t w = a.bits[((int64_t)(f0 + j) * a.H + y) * a.pitch + (x >> 5)];
              ok = (w >> (x & 31)) & 1u;
            } else {
              ok = !a.inall;   // behind the camera there is no border pixel: carved with inall_img
            }
          }
          if (a.use_nf) ok = ok && cz >= a.nf_lo && cz <= a.nf_hi;
          alive = ok;
        }
        if (__ballot(alive) == 0) break;
      }
    }
  }
  if (n < a.N) a.keep[n] = alive ? 1 : 0;
}

// ------------------------------------------------------------------- view
struct SeedViewArgs {
  const float* xyz;      // [M,3] the survivors
  const void* images;    // [F,H,W,3] uint8 or fp32
  const float* cams;     // [F,16]
  int64_t M;
  int F, H, W, u8;
  int32_t* cam_ind;      // [M]
  float* dirs;           // [M,3]
  float* color;          // [M,3]
  uint8_t* in_view;      // [M]
};

struct Unit {
  float x, y, z, n;   // d / (|d| + 1e-6), |d|
};

__device__ __forceinline__ Unit unit_to(const float p[3], const float c[3]) {
  const float dx = __fsub_rn(p[0], c[0]), dy = __fsub_rn(p[1], c[1]), dz = __fsub_rn(p[2], c[2]);
  const float n = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
  const float den = __fadd_rn(n, 1e-6f);
  return Unit{__fdiv_rn(dx, den), __fdiv_rn(dy, den), __fdiv_rn(dz, den), n};
}

__device__ __forceinline__ Row3 texel(const SeedViewArgs& a, int f, int y, int x) {
  const int64_t at = (((int64_t)f * a.H + y) * a.W + x) * 3;
  if (a.u8) {
    const uint8_t* q = static_cast<const uint8_t*>(a.images) + at;
    return Row3{__fdiv_rn((float)q[0], 255.0f), __fdiv_rn((float)q[1], 255.0f), __fdiv_rn((float)q[2], 255.0f)};
  }
  return *reinterpret_cast<const Row3*>(static_cast<const float*>(a.images) + at);
}

__global__ void __launch_bounds__(kSeedBlock) k_seed_view(SeedViewArgs a) {
  __shared__ float pos_s[kSeedTile * 3];
  __shared__ float dir_s[kSeedTile * 3];
  const int64_t m = (int64_t)blockIdx.x * kSeedBlock + threadIdx.x;
  const bool live = m < a.M;
  float p[3] = {0.f, 0.f, 0.f};
  if (live) {
    const Row3 r = reinterpret_cast<const Row3*>(a.xyz)[m];
    p[0] = r.x, p[1] = r.y, p[2] = r.z;
  }
  // nearest view: argmin_f |d| / 200 + (1.1 - d^ . camdir_f), lowest index on ties
  float best = 0.f;
  int best_f = 0;
  for (int f0 = 0; f0 < a.F; f0 += kSeedTile) {
    const int cnt = min(kSeedTile, a.F - f0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {   // one thread per camera of the tile: its position and centre-pixel ray
      const float* cam = a.cams + (int64_t)(f0 + threadIdx.x) * kCamRow;
      const Row3 d = pixel_dir((float)(a.W / 2), (float)(a.H / 2), cam, 1);
      const int t = threadIdx.x * 3;
      pos_s[t] = cam[9], pos_s[t + 1] = cam[10], pos_s[t + 2] = cam[11];
      dir_s[t] = d.x, dir_s[t + 1] = d.y, dir_s[t + 2] = d.z;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const Unit d = unit_to(p, pos_s + j * 3);
      const float* c = dir_s + j * 3;
      const float dot = __fadd_rn(__fadd_rn(__fmul_rn(d.x, c[0]), __fmul_rn(d.y, c[1])), __fmul_rn(d.z, c[2]));
      const float s = __fadd_rn(__fdiv_rn(d.n, 200.0f), __fsub_rn(1.1f, dot));
      if ((f0 + j == 0) || s < best) {
        best = s;
        best_f = f0 + j;
      }
    }
  }
  if (!live) return;
  const float* cam = a.cams + (int64_t)best_f * kCamRow;
  const Unit d = unit_to(p, cam + 9);
  float xc[3], u, v;
  world_to_cam(p, cam + 9, cam, xc);
  project(xc, cam, &u, &v);
  const bool seen = xc[2] > 0.f && in_image(u, v, a.W, a.H);
  Row3 c = Row3{0.f, 0.f, 0.f};
  if (seen) {   // bilinear, texel centres at + 0.5, taps clamped to the border
    const float sx = __fsub_rn(u, 0.5f), sy = __fsub_rn(v, 0.5f);
    const float fx = floorf(sx), fy = floorf(sy);
    const float wx = __fsub_rn(sx, fx), wy = __fsub_rn(sy, fy);
    const int x0 = max((int)fx, 0), x1 = min((int)fx + 1, a.W - 1);
    const int y0 = max((int)fy, 0), y1 = min((int)fy + 1, a.H - 1);
    const Row3 c00 = texel(a, best_f, y0, x0), c01 = texel(a, best_f, y0, x1);
    const Row3 c10 = texel(a, best_f, y1, x0), c11 = texel(a, best_f, y1, x1);
    c = Row3{lerp2(c00.x, c01.x, c10.x, c11.x, wx, wy), lerp2(c00.y, c01.y, c10.y, c11.y, wx, wy),
             lerp2(c00.z, c01.z, c10.z, c11.z, wx, wy)};
  }
  a.cam_ind[m] = best_f;
  reinterpret_cast<Row3*>(a.dirs)[m] = Row3{d.x, d.y, d.z};
  reinterpret_cast<Row3*>(a.color)[m] = c;
  a.in_view[m] = seen ? 1 : 0;
}

// Scratch of pnr_seed_mask: the scan's offsets [N + 1], then the scan's own.
inline size_t seed_offsets_bytes(int64_t N) { return ((size_t)(N + 1) * sizeof(int32_t) + 15) / 16 * 16; }

inline int check_frames(const char* who, int32_t F, int32_t H, int32_t W) {
  PNR_CHECK_ARG(F >= 1, "%s: F=%d frames (>= 1)", who, F);
  PNR_CHECK_ARG(H >= 1 && W >= 1, "%s: H=%d W=%d (H*W >= 1)", who, H, W);
  PNR_CHECK_ARG((int64_t)H * W <= (int64_t)1 << 31, "%s: H*W=%lld above 2^31", who, (long long)((int64_t)H * W));
  return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_alpha_bits(const void* alphas, int32_t alphas_u8, int32_t F, int32_t H, int32_t W, uint32_t* bits,
                              int32_t pitch_words, int64_t bits_words, void* stream) {
  PNR_CHECK_ARG(alphas && bits, "alpha_bits: null pointer");
  if (int rc = check_frames("alpha_bits", F, H, W)) return rc;
  PNR_CHECK_ARG(pitch_words == (W + 31) / 32, "alpha_bits: pitch of %d words, W=%d needs %d", pitch_words, W,
                (W + 31) / 32);
  const int64_t rows = (int64_t)F * H;
  PNR_CHECK_ARG(bits_words >= rows * pitch_words, "alpha_bits: bits holds %lld words, %lld needed",
                (long long)bits_words, (long long)(rows * pitch_words));
  AlphaBitsArgs a = {alphas, bits, rows, W, pitch_words, alphas_u8 != 0};
  const int64_t items = rows * cdiv(W, 64);
  hipLaunchKernelGGL(k_alpha_bits, dim3(grid_for(items, kSeedBlock / 64)), dim3(kSeedBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_seed_scratch_bytes(int64_t N, size_t* out) {
  PNR_CHECK_ARG(out, "seed_scratch_bytes: null out");
  PNR_CHECK_ARG(N >= 0 && N < (int64_t)1 << 31, "seed_scratch_bytes: N=%lld outside [0, 2^31)", (long long)N);
  *out = seed_offsets_bytes(N) + scan_scratch_bytes(N);
  return PNR_OK;
}

extern "C" int pnr_seed_mask(const float* xyz, int64_t N, const float* cams, int32_t F, int32_t H, int32_t W,
                             const uint32_t* bits, int32_t pitch_words, const float* ranges_host,
                             const float* near_far_host, int32_t inall_img, int32_t* keep, int32_t* src_idx,
                             int64_t out_cap, int32_t* count, void* scratch, size_t scratch_bytes, void* stream) {
  PNR_CHECK_ARG(xyz && cams && keep && src_idx && count && scratch, "seed_mask: null pointer");
  PNR_CHECK_ARG(N >= 1 && N < (int64_t)1 << 31, "seed_mask: N=%lld outside [1, 2^31)", (long long)N);
  if (int rc = check_frames("seed_mask", F, H, W)) return rc;
  PNR_CHECK_ARG(!bits || pitch_words == (W + 31) / 32, "seed_mask: pitch of %d words, W=%d needs %d", pitch_words, W,
                (W + 31) / 32);
  PNR_CHECK_ARG(out_cap >= N, "seed_mask: outputs hold %lld points, %lld may survive", (long long)out_cap,
                (long long)N);
  const size_t need = seed_offsets_bytes(N) + scan_scratch_bytes(N);
  PNR_CHECK_ARG(scratch_bytes >= need, "seed_mask: scratch too small (%zu < %zu)", scratch_bytes, need);
  SeedMaskArgs a = {};
  a.xyz = xyz, a.cams = cams, a.bits = bits, a.N = N;
  a.F = F, a.H = H, a.W = W, a.pitch = pitch_words;
  a.use_ranges = ranges_host && ranges_host[0] > -99.f;   // train_ft.py:678
  if (a.use_ranges)
    for (int i = 0; i < 3; ++i) a.lo[i] = ranges_host[i], a.hi[i] = ranges_host[3 + i];
  a.use_nf = near_far_host != nullptr;
  if (a.use_nf) a.nf_lo = near_far_host[0] - 1.0f, a.nf_hi = near_far_host[1];
  a.inall = inall_img != 0;
  a.views = bits || a.use_nf;
  a.keep = keep;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_seed_mask, dim3((unsigned)cdiv(N, kSeedBlock)), dim3(kSeedBlock), 0, st, a);
  PNR_LAUNCH_CHECK();
  // stable compaction: src_idx[offset[n]] = n for every survivor, count = their number
  int32_t* offsets = static_cast<int32_t*>(scratch);
  return exclusive_scan(keep, N, nullptr, offsets, N + 1, count, static_cast<char*>(scratch) + seed_offsets_bytes(N),
                        scratch_bytes - seed_offsets_bytes(N), st, 0, nullptr, src_idx);
}

extern "C" int pnr_seed_view(const float* xyz, int64_t M, const void* images, int32_t images_u8, const float* cams,
                             int32_t F, int32_t H, int32_t W, int32_t* cam_ind, float* dirs, float* color,
                             uint8_t* in_view, int64_t out_cap, void* stream) {
  PNR_CHECK_ARG(M >= 0 && M < (int64_t)1 << 31, "seed_view: M=%lld outside [0, 2^31)", (long long)M);
  if (int rc = check_frames("seed_view", F, H, W)) return rc;
  PNR_CHECK_ARG(out_cap >= M, "seed_view: outputs hold %lld points, M=%lld", (long long)out_cap, (long long)M);
  if (M == 0) return PNR_OK;
  PNR_CHECK_ARG(xyz && images && cams && cam_ind && dirs && color && in_view, "seed_view: null pointer");
  SeedViewArgs a = {xyz, images, cams, M, F, H, W, images_u8 != 0, cam_ind, dirs, color, in_view};
  hipLaunchKernelGGL(k_seed_view, dim3((unsigned)cdiv(M, kSeedBlock)), dim3(kSeedBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
