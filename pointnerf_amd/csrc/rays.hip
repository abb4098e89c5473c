// Ray batches on the device: the directions of a camera's pixels
// (data/data_utils.py:55-69, get_dtu_raydir) and one training batch of an
// image set resident on the device (nerf_synth360_ft_dataset.py:546-635: the
// pixel picks, their directions, their ground-truth colours, the bg coin).
// One thread per ray; the picks come from Philox4x32-10, a counter-based
// generator, so a batch depends on (seed, step) only -- not on the launch shape.
//
// Arithmetic: x = ((px + 0.5f) - cx) / fx in three correctly
// rounded fp32 operations, the rotation in fp64 on the widened fp32 entries,
// (x R[i][0] + y R[i][1]) + R[i][2] left to right without FMA, one rounding to
// fp32.  This file is built with -ffp-contract=off.
#include "pnr_common.h"

namespace pnr {

constexpr int kRBlock = 256;

// ------------------------------------------------------------------ Philox
struct U4 {
  uint32_t x, y, z, w;
};

__host__ __device__ inline uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 known-answer vectors).
__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// key = (seed lo, seed hi), counter = (i, step lo, step hi, stream)
__host__ __device__ inline U4 batch_random(int64_t seed, int64_t step, uint32_t i, uint32_t stream) {
  const uint64_t s = (uint64_t)seed, t = (uint64_t)step;
  return philox4x32_10(U4{i, (uint32_t)t, (uint32_t)(t >> 32), stream}, (uint32_t)s, (uint32_t)(s >> 32));
}

// -------------------------------------------------------------- directions
// (pixel_dir, the arithmetic above, lives in pnr_common.h: seed.hip shares it)
struct CamRaysArgs {
  const float* cam;      // the frame's row of the camera table
  const float* pixels;   // [R,2] (x, y) or nullptr: the H x W frame, x fastest
  int64_t R;
  int W, dir_norm;
  float* raydir;
  float* pixel_idx;      // optional
};

__global__ void __launch_bounds__(kRBlock) k_camera_rays(CamRaysArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.R; i += stride) {
    float px, py;
    if (a.pixels) {
      const Row2 p = reinterpret_cast<const Row2*>(a.pixels)[i];
      px = p.x;
      py = p.y;
    } else {
      px = (float)(i % a.W);
      py = (float)(i / a.W);
    }
    reinterpret_cast<Row3*>(a.raydir)[i] = pixel_dir(px, py, a.cam, a.dir_norm);
    if (a.pixel_idx) reinterpret_cast<Row2*>(a.pixel_idx)[i] = Row2{px, py};
  }
}

// ------------------------------------------------------------------ batches
struct RayBatchArgs {
  const void* images;       // [F,H,W,3] uint8 or fp32
  const float* cams;        // [F,16]
  const int64_t* state;     // {seed, step}: read only here (k_advance_step bumps it behind this launch)
  const int32_t* frame_dev; // optional
  int64_t R;
  int F, H, W, S;
  int frame;                // >= 0: this frame; < 0: frame_dev, or drawn when that is null
  int mode, bg_mode, images_u8, dir_norm;
  float* raydir;
  float* pixel_idx;
  float* gt;
  float* campos;
  float* camrot;
  float* bg;
  int32_t* frame_id;
};

__global__ void __launch_bounds__(kRBlock) k_ray_batch(RayBatchArgs a) {
  const int64_t seed = a.state[0], step = a.state[1];
  const U4 b = batch_random(seed, step, 0u, 1u);   // once per batch: patch origin, bg coin, frame
  int f = a.frame;
  if (f < 0) f = a.frame_dev ? a.frame_dev[0] : (int)mulhi32(b.w, (uint32_t)a.F);
  f = min(max(f, 0), a.F - 1);   // a device value is not the host's to check: never read outside the stack
  const float* cam = a.cams + (int64_t)f * kCamRow;
  const int W = a.W, H = a.H, S = a.S;
  int ox = 0, oy = 0;
  if (a.mode == PNR_RAYS_PATCH) {
    ox = (int)mulhi32(b.x, (uint32_t)(W - S + 1));
    oy = (int)mulhi32(b.y, (uint32_t)(H - S + 1));
  }
  if (blockIdx.x == 0 && threadIdx.x < kCamRow) {   // the batch's own rows
    const int t = threadIdx.x;
    if (t < 9) a.camrot[t] = cam[t];
    else if (t < 12) a.campos[t - 9] = cam[t];
    else if (t < 15) {
      if (a.bg_mode != PNR_BG_CALLER)
        a.bg[t - 12] = a.bg_mode == PNR_BG_WHITE ? 1.f
                       : a.bg_mode == PNR_BG_BLACK ? 0.f
                                                   : (b.z >= 0x80000000u ? 1.f : 0.f);
    } else {
      a.frame_id[0] = f;
    }
  }
  const int64_t frame_px = (int64_t)f * H * W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.R; i += stride) {
    int x, y;
    if (a.mode == PNR_RAYS_RANDOM) {
      const U4 r = batch_random(seed, step, (uint32_t)i, 0u);
      x = (int)mulhi32(r.x, (uint32_t)W);
      y = (int)mulhi32(r.y, (uint32_t)H);
    } else if (a.mode == PNR_RAYS_PATCH) {   // the reference's meshgrid order
      x = ox + (int)(i % S);
      y = oy + (int)(i / S);
    } else {
      x = (int)(i % W);
      y = (int)(i / W);
    }
    const float px = (float)x, py = (float)y;
    const int64_t at = (frame_px + (int64_t)y * W + x) * 3;
    Row3 c;
    if (a.images_u8) {
      const uint8_t* p = static_cast<const uint8_t*>(a.images) + at;
      c = Row3{__fdiv_rn((float)p[0], 255.0f), __fdiv_rn((float)p[1], 255.0f), __fdiv_rn((float)p[2], 255.0f)};
    } else {
      c = *reinterpret_cast<const Row3*>(static_cast<const float*>(a.images) + at);
    }
    reinterpret_cast<Row3*>(a.raydir)[i] = pixel_dir(px, py, cam, a.dir_norm);
    reinterpret_cast<Row2*>(a.pixel_idx)[i] = Row2{px, py};
    reinterpret_cast<Row3*>(a.gt)[i] = c;
  }
}

// Queued behind k_ray_batch on the same stream: every block of the batch has
// read the counter by the time this runs, so none of them sees the next step.
__global__ void k_advance_step(int64_t* state) { state[1] = state[1] + 1; }

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_camera_rays(const float* cams, int32_t F, int32_t frame, int32_t H, int32_t W,
                               const float* pixels, int64_t R, int32_t dir_norm, float* raydir, float* pixel_idx,
                               void* stream) {
  PNR_CHECK_ARG(cams && raydir, "camera_rays: null pointer");
  PNR_CHECK_ARG(F >= 1, "camera_rays: F=%d frames (>= 1)", F);
  PNR_CHECK_ARG(frame >= 0 && frame < F, "camera_rays: frame %d outside [0, %d)", frame, F);
  PNR_CHECK_ARG(H >= 1 && W >= 1, "camera_rays: H=%d W=%d (>= 1)", H, W);
  PNR_CHECK_ARG((int64_t)H * W <= (int64_t)1 << 31, "camera_rays: H*W=%lld above 2^31", (long long)((int64_t)H * W));
  PNR_CHECK_ARG(R >= 0 && R <= (int64_t)1 << 31, "camera_rays: R=%lld outside [0, 2^31]", (long long)R);
  PNR_CHECK_ARG(pixels || R == (int64_t)H * W, "camera_rays: R=%lld is not H*W=%lld and no pixel list was given",
                (long long)R, (long long)((int64_t)H * W));
  if (R == 0) return PNR_OK;
  CamRaysArgs a = {cams + (int64_t)frame * kCamRow, pixels, R, W, dir_norm != 0, raydir, pixel_idx};
  hipLaunchKernelGGL(k_camera_rays, dim3(grid_for(R, kRBlock)), dim3(kRBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}

extern "C" int pnr_ray_batch(const void* images, int32_t images_u8, const float* cams, int32_t F, int32_t H,
                             int32_t W, int64_t* state, int32_t frame, const int32_t* frame_dev, int32_t mode,
                             int32_t S, int32_t dir_norm, int32_t bg_mode, float* raydir, float* pixel_idx,
                             float* gt, float* campos, float* camrot, float* bg, int32_t* frame_id, void* stream) {
  PNR_CHECK_ARG(images && cams && state && raydir && pixel_idx && gt && campos && camrot && frame_id,
                "ray_batch: null pointer");
  PNR_CHECK_ARG(mode == PNR_RAYS_RANDOM || mode == PNR_RAYS_PATCH || mode == PNR_RAYS_FULL,
                "ray_batch: unknown mode %d", mode);
  PNR_CHECK_ARG(bg_mode >= PNR_BG_CALLER && bg_mode <= PNR_BG_RANDOM, "ray_batch: unknown bg mode %d", bg_mode);
  PNR_CHECK_ARG(bg || bg_mode == PNR_BG_CALLER, "ray_batch: null bg pointer");
  PNR_CHECK_ARG(F >= 1, "ray_batch: F=%d frames (>= 1)", F);
  PNR_CHECK_ARG(H >= 1 && W >= 1, "ray_batch: H=%d W=%d (>= 1)", H, W);
  PNR_CHECK_ARG((int64_t)H * W <= (int64_t)1 << 31, "ray_batch: H*W=%lld above 2^31", (long long)((int64_t)H * W));
  PNR_CHECK_ARG(frame < F, "ray_batch: frame %d outside [0, %d)", frame, F);
  int64_t R = (int64_t)H * W;
  if (mode != PNR_RAYS_FULL) {
    PNR_CHECK_ARG(S >= 1, "ray_batch: S=%d (>= 1)", S);
    PNR_CHECK_ARG(mode != PNR_RAYS_PATCH || S <= (H < W ? H : W), "ray_batch: patch S=%d above min(H, W)=%d", S,
                  H < W ? H : W);
    R = (int64_t)S * S;
    PNR_CHECK_ARG(R <= (int64_t)1 << 31, "ray_batch: R=S*S=%lld above 2^31", (long long)R);
  }
  RayBatchArgs a = {images, cams, state, frame_dev, R, F, H, W, S, frame, mode, bg_mode, images_u8 != 0,
                    dir_norm != 0, raydir, pixel_idx, gt, campos, camrot, bg, frame_id};
  hipLaunchKernelGGL(k_ray_batch, dim3(grid_for(R, kRBlock)), dim3(kRBlock), 0, as_stream(stream), a);
  PNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_advance_step, dim3(1), dim3(1), 0, as_stream(stream), state);
  PNR_LAUNCH_CHECK();
  return PNR_OK;
}
