// The plane background of bgmodel "plane" (DESIGN.md 35): per ray, the colour of
// the table plane as the source views see it.  mvs_utils.gen_bg_points /
// get_rayplane_cross (models/mvs/mvs_utils.py:380-408) intersect every ray with
// the plane, set_bg (models/mvs_points_volumetric_model.py:279-317) looks that
// point up in every source image, keeps the samples that look like the plane
// and that no neural point covers (homo_warp_fg_mask, mvs_utils.py:318-331) and
// takes their per-channel maximum; fill_invalid
// (neural_points_volumetric_model_ori.py:109-111) adds is_bg * bg_ray to the
// rendered colour.  Two kernels, one thread per point or ray: k_plane_fg marks
// the pixels the cloud covers in every view, k_plane_bg makes bg_ray and, when
// asked, finishes the frame.  Both stage the camera table through LDS in tiles;
// every lane reads the same camera, an LDS broadcast.
//
// Arithmetic: fp32, one rounding per operation, in the order written here
// (this file is built with -ffp-contract=off); tests/plane_bg_ref.py restates it
// in fp64.
#include "pnr_common.h"

namespace pnr {

constexpr int kPlaneBlock = 256;
constexpr int kPlaneTile = PNR_PLANE_CAM_TILE;

// (u, v) = (x / z fx + cx, y / z fy + cy): the reference's (xyz / z) @ K^T,
// texel centres at integer coordinates (pixel_pos of seed.hip is half a pixel
// off and multiplies before it divides).
__device__ __forceinline__ void plane_project(const float p[3], const float* cam, float* u, float* v) {
  float xc[3];
  world_to_cam(p, cam + 9, cam, xc);
  *u = __fadd_rn(__fmul_rn(__fdiv_rn(xc[0], xc[2]), cam[12]), cam[14]);
  *v = __fadd_rn(__fmul_rn(__fdiv_rn(xc[1], xc[2]), cam[13]), cam[15]);
}

// 0 <= u <= W - 1 and 0 <= v <= H - 1, both ends included; false for NaN.  No
// depth-sign test, as in the reference.
__device__ __forceinline__ bool plane_in_bounds(float u, float v, int W, int H) {
  return u >= 0.f && u <= (float)(W - 1) && v >= 0.f && v <= (float)(H - 1);
}

// -------------------------------------------------------------- foreground
struct PlaneFgArgs {
  const float* xyz;    // [N,3]
  const float* cams;   // [F,16]
  int64_t N;
  int F, H, W;
  uint8_t* fg;         // [F,H,W], zeroed by the caller
};

__global__ void __launch_bounds__(kPlaneBlock) k_plane_fg(PlaneFgArgs a) {
  __shared__ float cam_s[kPlaneTile * kCamRow];
  const int64_t n = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  const bool live = n < a.N;
  float p[3] = {0.f, 0.f, 0.f};
  if (live) {
    const Row3 r = reinterpret_cast<const Row3*>(a.xyz)[n];
    p[0] = r.x, p[1] = r.y, p[2] = r.z;
  }
  for (int f0 = 0; f0 < a.F; f0 += kPlaneTile) {
    const int cnt = min(kPlaneTile, a.F - f0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * kCamRow; i += kPlaneBlock) cam_s[i] = a.cams[(int64_t)f0 * kCamRow + i];
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < cnt; ++j) {
      float u, v;
      plane_project(p, cam_s + j * kCamRow, &u, &v);
      if (plane_in_bounds(u, v, a.W, a.H)) {   // ceil of a value in [0, W - 1] stays there
        const int x = (int)ceilf(u), y = (int)ceilf(v);
        a.fg[((int64_t)(f0 + j) * a.H + y) * a.W + x] = 1;   // every writer stores the same byte
      }
    }
  }
}

// -------------------------------------------------------------- background
struct PlaneBgArgs {
  const float* campos;   // [3] device
  const float* raydir;   // [R,3]
  const void* images;    // [F,H,W,3] uint8 or fp32
  const float* cams;     // [F,16]
  const uint8_t* fg;     // [F,H,W]
  int64_t R;
  int F, H, W, u8;
  float p0[3], nrm[3], color[3];
  float* bg;             // [R,3]
  const float* is_bg;    // [R] or nullptr: no epilogue
  float* ray_color;      // [R,3], += is_bg * bg
};

// One texel, or zero for the taps of padding_mode = 'zeros' (never loaded).
__device__ __forceinline__ Row3 plane_texel(const PlaneBgArgs& a, int f, int y, int x) {
  if (x >= a.W || y >= a.H) return Row3{0.f, 0.f, 0.f};
  const int64_t at = (((int64_t)f * a.H + y) * a.W + x) * 3;
  if (a.u8) {
    const uint8_t* q = static_cast<const uint8_t*>(a.images) + at;
    return Row3{__fdiv_rn((float)q[0], 255.0f), __fdiv_rn((float)q[1], 255.0f), __fdiv_rn((float)q[2], 255.0f)};
  }
  return *reinterpret_cast<const Row3*>(static_cast<const float*>(a.images) + at);
}

__global__ void __launch_bounds__(kPlaneBlock) k_plane_bg(PlaneBgArgs a) {
  __shared__ float cam_s[kPlaneTile * kCamRow];
  const int64_t r = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  const bool live = r < a.R;
  // the plane point of the ray, or the world origin (mvs_utils.py:406-407)
  float p[3] = {0.f, 0.f, 0.f};
  if (live) {
    const Row3 d = reinterpret_cast<const Row3*>(a.raydir)[r];
    const float c[3] = {a.campos[0], a.campos[1], a.campos[2]};
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(a.nrm[0], d.x), __fmul_rn(a.nrm[1], d.y)), __fmul_rn(a.nrm[2], d.z));
    if (dot >= 1e-3f) {
      const float w0 = __fsub_rn(c[0], a.p0[0]), w1 = __fsub_rn(c[1], a.p0[1]), w2 = __fsub_rn(c[2], a.p0[2]);
      const float nw = __fadd_rn(__fadd_rn(__fmul_rn(a.nrm[0], w0), __fmul_rn(a.nrm[1], w1)), __fmul_rn(a.nrm[2], w2));
      const float fac = __fdiv_rn(-nw, dot);
      p[0] = ray_at(c[0], d.x, fac), p[1] = ray_at(c[1], d.y, fac), p[2] = ray_at(c[2], d.z, fac);
    }
  }
  float lo[3], hi[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) lo[i] = __fsub_rn(a.color[i], 0.03f), hi[i] = __fadd_rn(a.color[i], 0.03f);
  Row3 best = Row3{0.f, 0.f, 0.f};
  bool any = false;
  for (int f0 = 0; f0 < a.F; f0 += kPlaneTile) {
    const int cnt = min(kPlaneTile, a.F - f0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * kCamRow; i += kPlaneBlock) cam_s[i] = a.cams[(int64_t)f0 * kCamRow + i];
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < cnt; ++j) {
      const int f = f0 + j;
      float u, v;
      plane_project(p, cam_s + j * kCamRow, &u, &v);
      if (!plane_in_bounds(u, v, a.W, a.H)) continue;
      if (a.fg[((int64_t)f * a.H + (int)ceilf(v)) * a.W + (int)ceilf(u)] != 0) continue;   // a neural point covers it
      // bilinear with texel centres at the integers; x0 + 1 = W happens at u = W - 1 only, with weight 0
      const float fx = floorf(u), fy = floorf(v);
      const float wx = __fsub_rn(u, fx), wy = __fsub_rn(v, fy);
      const int x0 = (int)fx, y0 = (int)fy;
      const Row3 c00 = plane_texel(a, f, y0, x0), c01 = plane_texel(a, f, y0, x0 + 1);
      const Row3 c10 = plane_texel(a, f, y0 + 1, x0), c11 = plane_texel(a, f, y0 + 1, x0 + 1);
      const Row3 s = Row3{lerp2(c00.x, c01.x, c10.x, c11.x, wx, wy), lerp2(c00.y, c01.y, c10.y, c11.y, wx, wy),
                          lerp2(c00.z, c01.z, c10.z, c11.z, wx, wy)};
      const bool fit = s.x >= lo[0] && s.x <= hi[0] && s.y >= lo[1] && s.y <= hi[1] && s.z >= lo[2] && s.z <= hi[2];
      if (!fit) continue;
      best = any ? Row3{fmaxf(best.x, s.x), fmaxf(best.y, s.y), fmaxf(best.z, s.z)} : s;
      any = true;
    }
  }
  if (!live) return;
  reinterpret_cast<Row3*>(a.bg)[r] = best;
  if (a.is_bg) {   // fill_invalid: colour += is_bg * bg_ray
    const float w = a.is_bg[r];
    Row3* out = reinterpret_cast<Row3*>(a.ray_color) + r;
    const Row3 c = *out;
    *out = Row3{__fadd_rn(c.x, __fmul_rn(w, best.x)), __fadd_rn(c.y, __fmul_rn(w, best.y)),
                __fadd_rn(c.z, __fmul_rn(w, best.z))};
  }
}

inline int check_plane_frames(const char* who, int32_t F, int32_t H, int32_t W) {
  PNR_CHECK_ARG(F >= 1, "%s: F=%d frames (>= 1)", who, F);
  PNR_CHECK_ARG(H >= 1 && W >= 1, "%s: H=%d W=%d (H*W >= 1)", who, H, W);
  PNR_CHECK_ARG((int64_t)H * W <= (int64_t)1 << 31, "%s: H*W=%lld above 2^31", who, (long long)((int64_t)H * W));
  return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_plane_fg_masks(const float* xyz, int64_t N, const float* cams, int32_t F, int32_t H, int32_t W,
                                  uint8_t* fg, int64_t fg_bytes, void* stream) {
  PNR_CHECK_ARG(N >= 0 && N < (int64_t)1 << 31, "plane_fg_masks: N=%lld outside [0, 2^31)", (long long)N);
  if (int rc = check_plane_frames("plane_fg_masks", F, H, W)) return rc;
  PNR_CHECK_ARG(fg_bytes >= (int64_t)F * H * W, "plane_fg_masks: fg holds %lld bytes, %lld needed", (long long)fg_bytes,
                (long long)((int64_t)F * H * W));
  if (N == 0) return PNR_OK;
  PNR_CHECK_ARG(xyz && cams && fg, "plane_fg_masks: null pointer");
  PlaneFgArgs a = {xyz, cams, N, F, H, W, fg};
  hipLaunchKernelGGL(k_plane_fg, dim3((unsigned)cdiv(N, kPlaneBlock)), dim3(kPlaneBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_plane_bg(const float* campos, const float* raydir, int64_t R, const void* images, int32_t images_u8,
                            const float* cams, int32_t F, int32_t H, int32_t W, const uint8_t* fg, int64_t fg_bytes,
                            const float* plane_pnt_host, const float* plane_normal_host,
                            const float* plane_color_host, float* bg, int64_t bg_cap, const float* is_bg,
                            float* ray_color, void* stream) {
  PNR_CHECK_ARG(R >= 0 && R < (int64_t)1 << 31, "plane_bg: R=%lld outside [0, 2^31)", (long long)R);
  if (int rc = check_plane_frames("plane_bg", F, H, W)) return rc;
  PNR_CHECK_ARG(plane_pnt_host && plane_normal_host && plane_color_host, "plane_bg: null plane");
  PNR_CHECK_ARG(fg_bytes >= (int64_t)F * H * W, "plane_bg: fg holds %lld bytes, %lld needed", (long long)fg_bytes,
                (long long)((int64_t)F * H * W));
  PNR_CHECK_ARG(bg_cap >= R, "plane_bg: outputs hold %lld rays, R=%lld", (long long)bg_cap, (long long)R);
  PNR_CHECK_ARG((is_bg == nullptr) == (ray_color == nullptr), "plane_bg: is_bg and ray_color go together");
  if (R == 0) return PNR_OK;
  PNR_CHECK_ARG(campos && raydir && images && cams && fg && bg, "plane_bg: null pointer");
  PlaneBgArgs a = {};
  a.campos = campos, a.raydir = raydir, a.images = images, a.cams = cams, a.fg = fg, a.R = R;
  a.F = F, a.H = H, a.W = W, a.u8 = images_u8 != 0;
  for (int i = 0; i < 3; ++i)
    a.p0[i] = plane_pnt_host[i], a.nrm[i] = plane_normal_host[i], a.color[i] = plane_color_host[i];
  a.bg = bg, a.is_bg = is_bg, a.ray_color = ray_color;
  hipLaunchKernelGGL(k_plane_bg, dim3((unsigned)cdiv(R, kPlaneBlock)), dim3(kPlaneBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
