// Posed depth maps fused into a seed cloud: the geometric part
// of the reference's gen_points, filter_by_masks_gpu (models/mvs/
// filter_utils.py:157-291).  Every valid pixel of every view is projected into
// every other view, brought back through that view's depth, and kept when
// enough views agree; the agreeing depths are averaged.  Two kernels:
// k_depth_fuse, one thread per reference pixel looping over the source views
// (cameras staged through LDS in tiles, every lane reads the same camera: an
// LDS broadcast), and k_depth_points, one thread per survivor of the scan's
// list.
//
// Arithmetic: fp32, one rounding per operation, in the order written here
// (this file is built with -ffp-contract=off); tests/fuse_ref.py restates it
// in fp64.
#include "pnr_common.h"

namespace pnr {

constexpr int kFuseBlock = 256;
constexpr int kFuseTileW = 16;   // 16 x 16 pixels per block; 32 x 8 measured 1 % slower
constexpr int kFuseTileH = kFuseBlock / kFuseTileW;
constexpr int kFuseCams = PNR_SEED_CAM_TILE;

struct DepthFuseArgs {
  const float* depths;   // [F,H,W]
  const float* conf;     // [F,H,W] or nullptr
  const uint8_t* mask;   // [F,H,W] or nullptr
  const float* cams;     // [F,16]
  int F, H, W;
  int tiles_x, tiles_y;
  float pix_thresh, rel_thresh, conf_thresh;
  int geo_cnsst_num, use_ranges;
  float lo[3], hi[3];
  float* depth_avg;      // [F,H,W]
  int32_t* count;        // [F,H,W]
  int32_t* visible;      // [F,H,W]
  int32_t* keep;         // [F*H*W] 1 = survivor
};

__device__ __forceinline__ bool depth_ok(float d) {   // false for NaN, +-inf, d <= 0
  return d > 0.f && d < __builtin_inff();
}

// The world point of the continuous pixel position (x, y) of a view at depth d:
// R ((x - cx0) / fx d, (y - cy0) / fy d, d) + campos, each row summed left to right.
__device__ __forceinline__ void pixel_point(float x, float y, float d, const float* cam, float p[3]) {
  const float a = __fmul_rn(__fdiv_rn(__fsub_rn(x, cam[14]), cam[12]), d);
  const float b = __fmul_rn(__fdiv_rn(__fsub_rn(y, cam[15]), cam[13]), d);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    p[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(cam[k * 3], a), __fmul_rn(cam[k * 3 + 1], b)),
                               __fmul_rn(cam[k * 3 + 2], d)),
                     cam[9 + k]);
}

// One block per tile of kFuseTileW x kFuseTileH pixels of one reference view:
// neighbouring pixels land on neighbouring source texels, so the four gathers
// of a wave share cache lines.
__global__ void __launch_bounds__(kFuseBlock) k_depth_fuse(DepthFuseArgs a) {
  __shared__ float cam_s[kFuseCams * kCamRow];
  const int64_t per_view = (int64_t)a.tiles_x * a.tiles_y;
  const int r = (int)(blockIdx.x / per_view);
  const int tile = (int)(blockIdx.x % per_view);
  const int i = (tile % a.tiles_x) * kFuseTileW + (int)threadIdx.x % kFuseTileW;
  const int j = (tile / a.tiles_x) * kFuseTileH + (int)threadIdx.x / kFuseTileW;
  const bool in_frame = i < a.W && j < a.H;
  const int64_t at = ((int64_t)r * a.H + j) * a.W + i;
  const float* cam_r = a.cams + (int64_t)r * kCamRow;   // uniform: scalar loads
  const float x = __fadd_rn((float)i, 0.5f), y = __fadd_rn((float)j, 0.5f);
  const float d = in_frame ? a.depths[at] : 0.f;
  const bool valid = in_frame && depth_ok(d);
  float p[3] = {0.f, 0.f, 0.f};
  if (valid) pixel_point(x, y, d, cam_r, p);
  int count = 0, visible = 0;
  float sum = 0.f;
  if (__syncthreads_or(valid)) {   // a tile without a valid pixel tests nothing
    for (int f0 = 0; f0 < a.F; f0 += kFuseCams) {
      const int cnt = min(kFuseCams, a.F - f0);
      if (f0) __syncthreads();   // the previous tile is free
      for (int k = threadIdx.x; k < cnt * kCamRow; k += kFuseBlock) cam_s[k] = a.cams[(int64_t)f0 * kCamRow + k];
      __syncthreads();
      if (__ballot(valid) == 0) continue;   // this wave only keeps the barriers
      for (int t = 0; t < cnt; ++t) {
        const int s = f0 + t;
        if (s == r) continue;
        const float* cam = cam_s + t * kCamRow;
        float xc[3], u = 0.f, v = 0.f;
        bool vis = false;
        if (valid) {
          world_to_cam(p, cam + 9, cam, xc);
          project(xc, cam, &u, &v);
          vis = xc[2] > 0.f && in_image(u, v, a.W, a.H);
        }
        if (__ballot(vis) == 0) continue;   // nobody of this wave sees view s: no sampling
        if (!vis) continue;
        ++visible;
        // bilinear, texel centres at + 0.5, taps clamped to the border (k_seed_view's sampler)
        const float sx = __fsub_rn(u, 0.5f), sy = __fsub_rn(v, 0.5f);
        const float fx = floorf(sx), fy = floorf(sy);
        const float wx = __fsub_rn(sx, fx), wy = __fsub_rn(sy, fy);
        const int x0 = max((int)fx, 0), x1 = min((int)fx + 1, a.W - 1);
        const int y0 = max((int)fy, 0), y1 = min((int)fy + 1, a.H - 1);
        const float* img = a.depths + (int64_t)s * a.H * a.W;
        const float t00 = img[(int64_t)y0 * a.W + x0], t01 = img[(int64_t)y0 * a.W + x1];
        const float t10 = img[(int64_t)y1 * a.W + x0], t11 = img[(int64_t)y1 * a.W + x1];
        if (!(depth_ok(t00) && depth_ok(t01) && depth_ok(t10) && depth_ok(t11))) continue;
        const float ds = lerp2(t00, t01, t10, t11, wx, wy);
        float q[3], c2[3], u2, v2;
        pixel_point(u, v, ds, cam, q);
        world_to_cam(q, cam_r + 9, cam_r, c2);
        project(c2, cam_r, &u2, &v2);
        const float du = __fsub_rn(u2, x), dv = __fsub_rn(v2, y);
        const float dist = __fsqrt_rn(__fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv)));
        const float rel = __fdiv_rn(fabsf(__fsub_rn(c2[2], d)), d);
        if (c2[2] > 0.f && dist < a.pix_thresh && rel < a.rel_thresh) {
          ++count;
          sum = __fadd_rn(sum, c2[2]);
        }
      }
    }
  }
  if (!in_frame) return;
  const float avg = valid ? __fdiv_rn(__fadd_rn(d, sum), (float)(count + 1)) : 0.f;
  bool keep = valid && (a.F == 1 || count >= a.geo_cnsst_num);
  if (a.conf) keep = keep && a.conf[at] > a.conf_thresh;
  if (a.mask) keep = keep && a.mask[at] != 0;
  if (keep && a.use_ranges) {
    float w[3];
    pixel_point(x, y, avg, cam_r, w);
    keep = w[0] >= a.lo[0] && w[0] <= a.hi[0] && w[1] >= a.lo[1] && w[1] <= a.hi[1] && w[2] >= a.lo[2] &&
           w[2] <= a.hi[2];
  }
  a.depth_avg[at] = avg;
  a.count[at] = count;
  a.visible[at] = visible;
  a.keep[at] = keep ? 1 : 0;
}

// ----------------------------------------------------------------- points
struct DepthPointsArgs {
  const int32_t* src;         // [M] the scan's list: flat pixels of [F,H,W]
  const float* depth_avg;     // [F,H,W]
  const int32_t* count_map;   // [F,H,W]
  const float* conf;          // [F,H,W] or nullptr: 1
  const float* cams;
  int64_t M;
  int H, W;
  int geo_cnsst_num, reassign;
  float factor[10];           // 1 - 1 / 1.14869^k, k = 1 .. 10
  float* xyz;                 // [M,3]
  float* conf_out;            // [M]
  int64_t* src_pixel;         // [M]
  int32_t* count_out;         // [M]
};

__global__ void __launch_bounds__(kFuseBlock) k_depth_points(DepthPointsArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
  if (m >= a.M) return;
  const int32_t at = a.src[m];
  const int r = at / (a.H * a.W), rem = at % (a.H * a.W);
  const int j = rem / a.W, i = rem % a.W;
  float p[3];
  pixel_point(__fadd_rn((float)i, 0.5f), __fadd_rn((float)j, 0.5f), a.depth_avg[at], a.cams + (int64_t)r * kCamRow, p);
  const int count = a.count_map[at];
  float c = a.conf ? a.conf[at] : 1.f;
  if (a.reassign) c = __fmul_rn(c, a.factor[min(max(count - a.geo_cnsst_num + 1, 1), 10) - 1]);
  reinterpret_cast<Row3*>(a.xyz)[m] = Row3{p[0], p[1], p[2]};
  a.conf_out[m] = c;
  a.src_pixel[m] = at;
  a.count_out[m] = count;
}

// Scratch of pnr_depth_fuse: the scan's offsets [n + 1], then the scan's own.
inline size_t fuse_offsets_bytes(int64_t n) { return ((size_t)(n + 1) * sizeof(int32_t) + 15) / 16 * 16; }

inline int check_maps(const char* who, int32_t F, int32_t H, int32_t W) {
  PNR_CHECK_ARG(F >= 1, "%s: F=%d frames (>= 1)", who, F);
  PNR_CHECK_ARG(H >= 1 && W >= 1, "%s: H=%d W=%d (H, W >= 1)", who, H, W);
  PNR_CHECK_ARG((int64_t)F * H * W < (int64_t)1 << 31, "%s: F*H*W=%lld not below 2^31", who,
                (long long)((int64_t)F * H * W));
  return PNR_OK;
}

inline int check_params(const char* who, const pnr_fuse_params* q) {
  PNR_CHECK_ARG(q, "%s: null params", who);
  PNR_CHECK_ARG(q->pix_thresh > 0.f && q->rel_thresh > 0.f, "%s: pix_thresh=%g rel_thresh=%g (> 0)", who,
                (double)q->pix_thresh, (double)q->rel_thresh);
  PNR_CHECK_ARG(q->geo_cnsst_num >= 0, "%s: geo_cnsst_num=%d (>= 0)", who, q->geo_cnsst_num);
  return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_depth_fuse_scratch_bytes(int32_t F, int32_t H, int32_t W, size_t* out) {
  PNR_CHECK_ARG(out, "depth_fuse_scratch_bytes: null out");
  if (int rc = check_maps("depth_fuse_scratch_bytes", F, H, W)) return rc;
  const int64_t n = (int64_t)F * H * W;
  *out = fuse_offsets_bytes(n) + scan_scratch_bytes(n);
  return PNR_OK;
}

extern "C" int pnr_depth_fuse(const float* depths, const float* conf, const uint8_t* mask, const float* cams,
                              int32_t F, int32_t H, int32_t W, const pnr_fuse_params* params_host, float* depth_avg,
                              int32_t* count, int32_t* visible, int32_t* keep, int32_t* src, int64_t cap,
                              int32_t* count_dev, void* scratch, size_t scratch_bytes, void* stream) {
  PNR_CHECK_ARG(depths && cams && depth_avg && count && visible && keep && src && count_dev && scratch,
                "depth_fuse: null pointer");
  if (int rc = check_maps("depth_fuse", F, H, W)) return rc;
  if (int rc = check_params("depth_fuse", params_host)) return rc;
  const int64_t n = (int64_t)F * H * W;
  PNR_CHECK_ARG(cap >= n, "depth_fuse: outputs hold %lld pixels, %lld may survive", (long long)cap, (long long)n);
  const size_t need = fuse_offsets_bytes(n) + scan_scratch_bytes(n);
  PNR_CHECK_ARG(scratch_bytes >= need, "depth_fuse: scratch too small (%zu < %zu)", scratch_bytes, need);
  DepthFuseArgs a = {};
  a.depths = depths, a.conf = conf, a.mask = mask, a.cams = cams;
  a.F = F, a.H = H, a.W = W;
  a.tiles_x = (int)cdiv(W, kFuseTileW), a.tiles_y = (int)cdiv(H, kFuseTileH);
  a.pix_thresh = params_host->pix_thresh, a.rel_thresh = params_host->rel_thresh;
  a.conf_thresh = params_host->conf_thresh, a.geo_cnsst_num = params_host->geo_cnsst_num;
  a.use_ranges = params_host->ranges[0] > -99.f;   // as pnr_seed_mask
  for (int k = 0; k < 3; ++k) a.lo[k] = params_host->ranges[k], a.hi[k] = params_host->ranges[3 + k];
  a.depth_avg = depth_avg, a.count = count, a.visible = visible, a.keep = keep;
  const int64_t blocks = (int64_t)a.tiles_x * a.tiles_y * F;   // every tile holds a pixel: <= F H W < 2^31
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_depth_fuse, dim3((unsigned)blocks), dim3(kFuseBlock), 0, st, a);
  PNR_LAUNCH_CHECK();
  // stable compaction: src[offset[n]] = n for every survivor, count_dev = their number
  int32_t* offsets = static_cast<int32_t*>(scratch);
  const size_t off = fuse_offsets_bytes(n);
  return exclusive_scan(keep, n, nullptr, offsets, n + 1, count_dev, static_cast<char*>(scratch) + off,
                        scratch_bytes - off, st, 0, nullptr, src);
}

extern "C" int pnr_depth_points(const int32_t* src, int64_t M, const float* depth_avg, const int32_t* count_map,
                                const float* conf, const float* cams, int32_t F, int32_t H, int32_t W,
                                const pnr_fuse_params* params_host, float* xyz, float* conf_out, int64_t* src_pixel,
                                int32_t* count_out, int64_t out_cap, void* stream) {
  if (int rc = check_maps("depth_points", F, H, W)) return rc;
  if (int rc = check_params("depth_points", params_host)) return rc;
  PNR_CHECK_ARG(M >= 0 && M <= (int64_t)F * H * W, "depth_points: M=%lld outside [0, F*H*W=%lld]", (long long)M,
                (long long)((int64_t)F * H * W));
  PNR_CHECK_ARG(out_cap >= M, "depth_points: outputs hold %lld points, M=%lld", (long long)out_cap, (long long)M);
  if (M == 0) return PNR_OK;
  PNR_CHECK_ARG(src && depth_avg && count_map && cams && xyz && conf_out && src_pixel && count_out,
                "depth_points: null pointer");
  DepthPointsArgs a = {};
  a.src = src, a.depth_avg = depth_avg, a.count_map = count_map, a.conf = conf, a.cams = cams;
  a.M = M, a.H = H, a.W = W;
  a.geo_cnsst_num = params_host->geo_cnsst_num, a.reassign = params_host->reassign_conf != 0;
  double pw = 1.0;
  for (int k = 0; k < 10; ++k) {   // filter_utils.py:296, 1.14869 = 2^(1/5)
    pw *= 1.14869;
    a.factor[k] = (float)(1.0 - 1.0 / pw);
  }
  a.xyz = xyz, a.conf_out = conf_out, a.src_pixel = src_pixel, a.count_out = count_out;
  hipLaunchKernelGGL(k_depth_points, dim3((unsigned)cdiv(M, kFuseBlock)), dim3(kFuseBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
