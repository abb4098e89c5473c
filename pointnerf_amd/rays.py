"""Ray batches made on the device: "render this camera" and "give me the next
training batch of this image set".

``camera_rays`` is get_dtu_raydir (data/data_utils.py:55-69) on pnr_camera_rays;
``FrameSet`` keeps an image stack and its cameras on the device and returns the
reference dataset's item (data/nerf_synth360_ft_dataset.py:546-647) from one
pnr_ray_batch call: the pixel picks, their directions, their ground-truth
colours and the ``bg_color == 'random'`` coin, drawn from a counter-based
generator whose step counter lives on the device.  After the
first call ``FrameSet.sample(out=...)`` reads nothing on the host, waits for
nothing and allocates nothing, so it can be captured in a HIP graph: every
replay draws the next batch.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

RAYS_RANDOM, RAYS_PATCH, RAYS_FULL = 0, 1, 2
MODES = {"random": RAYS_RANDOM, "patch": RAYS_PATCH, "full": RAYS_FULL, "no_crop": RAYS_FULL,
         "full_image": RAYS_FULL}
REFUSED_MODES = {
    "random2": "it gathers unfiltered colours at fractional pixels",
    "proportional_random": "the reference itself raises for it (no gt_mask)",
}
BG_CALLER, BG_WHITE, BG_BLACK, BG_RANDOM = 0, 1, 2, 3
BG_MODES = {"white": BG_WHITE, "black": BG_BLACK, "random": BG_RANDOM}


def mode_code(mode: str) -> int:
    """PNR_RAYS_* of a reference ``random_sample`` name; the two modes this
    package does not build are refused by name."""
    if mode in REFUSED_MODES:
        raise L.PnrError(f"random_sample '{mode}' is not supported: {REFUSED_MODES[mode]}")
    if mode not in MODES:
        raise L.PnrError(f"unknown random_sample '{mode}' (one of {sorted(MODES)})")
    return MODES[mode]


def _tensor(a) -> torch.Tensor:
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def camera_table(campos, camrot, intrinsics, F: int, H: int, W: int, device) -> torch.Tensor:
    """cams [F,16] fp32 on ``device``: camrotc2w row-major (9), campos (3), fx,
    fy, cx, cy.  intrinsics: [3,3], [F,3,3], or a focal length (cx = W/2, cy =
    H/2).  Every value is rounded to fp32 once, from the dtype it came in."""
    K = _tensor(intrinsics).detach()
    if K.dim() == 0:
        f = K.double().reshape(1)
        vals = torch.stack([f, f, torch.full_like(f, W / 2), torch.full_like(f, H / 2)], -1)
    else:
        K = K.reshape(-1, 3, 3)
        vals = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], -1)
    if vals.shape[0] not in (1, F):
        raise L.PnrError(f"intrinsics for {vals.shape[0]} frames, cameras for {F}")
    parts = [_tensor(camrot).detach().reshape(F, 9), _tensor(campos).detach().reshape(F, 3), vals.expand(F, 4)]
    return torch.cat([p.to(device).float() for p in parts], 1).contiguous()


def camera_rays(intrinsic, camrotc2w, H: int, W: int, pixels=None, dir_norm=False, device=None,
                return_pixels: bool = False):
    """raydir [R,3] (device, fp32) of one camera: the whole H x W frame in
    row-major order, or the pixels [R,2] (x, y) given.  intrinsic: [3,3] or a
    focal length with cx = W/2, cy = H/2.  With return_pixels: (raydir,
    pixel_idx [R,2])."""
    if device is None:
        device = camrotc2w.device if torch.is_tensor(camrotc2w) and camrotc2w.is_cuda else "cuda"
    device = torch.device(device)
    L.require_gpu()
    H, W = int(H), int(W)
    cams = camera_table(torch.zeros(3), camrotc2w, intrinsic, 1, H, W, device)
    if pixels is not None:
        pixels = _tensor(pixels).to(device).float().reshape(-1, 2).contiguous()
        R = pixels.shape[0]
    else:
        R = max(H, 0) * max(W, 0)
    raydir = torch.empty((R, 3), dtype=torch.float32, device=device)
    pidx = torch.empty((R, 2), dtype=torch.float32, device=device) if return_pixels else None
    L.check(L.lib().pnr_camera_rays(L.ptr(cams), 1, 0, H, W, L.ptr(pixels), R, int(bool(dir_norm)), L.ptr(raydir),
                                    L.ptr(pidx), L.stream_ptr(device)), "pnr_camera_rays")
    return (raydir, pidx) if return_pixels else raydir


class FrameSet:
    """An image set and its cameras, resident on the device.

    images [F,H,W,3] uint8 or float (numpy or torch; uploaded once, uint8 kept
    as uint8, floats as fp32); c2w [F,4,4] or (campos [F,3], camrotc2w
    [F,3,3]); intrinsics [3,3] or [F,3,3]; near / far host scalars; bg_color
    'white', 'black', 'random' (a coin per batch) or a caller tensor of any
    channel count (e.g. a learned 128-channel parameter), passed through."""

    def __init__(self, images, c2w, intrinsics, near, far, bg_color="white", dir_norm=0, seed=0, device="cuda"):
        L.require_gpu()
        self.device = dev = torch.device(device)
        img = _tensor(images)
        if img.dim() != 4 or img.shape[-1] != 3 or img.shape[0] < 1:
            raise L.PnrError(f"images must be [F,H,W,3], got {tuple(img.shape)}")
        if img.dtype != torch.uint8:
            if not img.dtype.is_floating_point:
                raise L.PnrError(f"images must be uint8 or float, got {img.dtype}")
            img = img.float()
        self.images = img.to(dev).contiguous()
        self.F, self.h, self.w = (int(s) for s in img.shape[:3])
        if isinstance(c2w, (tuple, list)) and len(c2w) == 2:
            campos, camrot = _tensor(c2w[0]), _tensor(c2w[1])
        else:
            m = _tensor(c2w).reshape(-1, 4, 4)
            campos, camrot = m[:, :3, 3], m[:, :3, :3]
        if campos.reshape(-1, 3).shape[0] != self.F or camrot.reshape(-1, 3, 3).shape[0] != self.F:
            raise L.PnrError(f"{self.F} images, {campos.reshape(-1, 3).shape[0]} cameras")
        self.cams = camera_table(campos, camrot, intrinsics, self.F, self.h, self.w, dev)
        K = _tensor(intrinsics).detach().reshape(-1, 3, 3)
        self.intrinsics = K.to(dev).float().contiguous()       # [1,3,3] shared or [F,3,3]
        self.near, self.far = float(near), float(far)
        self.dir_norm = int(dir_norm)
        if isinstance(bg_color, str):
            if bg_color not in BG_MODES:
                raise L.PnrError(f"bg_color '{bg_color}': one of {sorted(BG_MODES)} or a tensor")
            self.bg_mode, self.bg_tensor = BG_MODES[bg_color], None
        elif torch.is_tensor(bg_color):
            self.bg_mode, self.bg_tensor = BG_CALLER, bg_color
        else:
            raise L.PnrError("bg_color: 'white', 'black', 'random' or a tensor")
        self._seed = int(seed)
        self._state = torch.tensor([self._seed, 0], dtype=torch.int64, device=dev)
        # frame(i) draws its coin at step i of a counter of its own: evaluation
        # never moves the training batches
        self._eval_state = torch.tensor([self._seed, 0], dtype=torch.int64, device=dev)

    def __len__(self):
        return self.F

    # ------------------------------------------------------------- the counter
    @property
    def seed(self) -> int:
        return self._seed

    @seed.setter
    def seed(self, v: int):
        self._seed = int(v)
        self._state[0] = self._seed
        self._eval_state[0] = self._seed

    @property
    def step(self) -> int:
        """Batches drawn so far (the one host read of this class)."""
        return int(self._state[1].item())

    @step.setter
    def step(self, v: int):
        self._state[1] = int(v)

    # ----------------------------------------------------------------- batches
    def _rays(self, code: int, size) -> tuple[int, int]:
        if code == RAYS_FULL:
            return 0, self.h * self.w
        S = int(size) if size is not None else 0
        if S < 1:
            raise L.PnrError(f"sample size {size}: at least 1")
        if code == RAYS_PATCH and S > min(self.h, self.w):
            raise L.PnrError(f"patch size {S} above min(h, w) = {min(self.h, self.w)}")
        return S, S * S

    def alloc(self, R: int) -> dict:
        """The tensors of one item of R rays (what ``out=`` reuses)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        item = dict(campos=torch.empty((1, 3), **f32), camrotc2w=torch.empty((1, 3, 3), **f32),
                    raydir=torch.empty((1, R, 3), **f32), pixel_idx=torch.empty((1, R, 2), **f32),
                    gt_image=torch.empty((1, R, 3), **f32),
                    id=torch.empty(1, dtype=torch.int32, device=self.device))
        if self.bg_mode != BG_CALLER:
            item["bg_color"] = torch.empty((1, 3), **f32)
        if self.intrinsics.shape[0] > 1:
            item["intrinsic"] = torch.empty((1, 3, 3), **f32)
        return item

    def _batch(self, state, code, S, R, frame, out):
        if out is None:
            out = self.alloc(R)
        elif tuple(out["raydir"].shape) != (1, R, 3):
            raise L.PnrError(f"out= holds {out['raydir'].shape[1]} rays, this batch has {R}")
        frame_dev = None
        if frame is None:
            frame_i = -1
        elif torch.is_tensor(frame):
            if not frame.is_cuda or frame.dtype != torch.int32 or frame.numel() != 1:
                raise L.PnrError("frame: an int, None or a device int32 tensor of one element")
            frame_i, frame_dev = -1, frame
        else:
            frame_i = int(frame)
            if not 0 <= frame_i < self.F:
                raise L.PnrError(f"frame {frame_i} outside [0, {self.F})")
        bg = out.get("bg_color") if self.bg_mode != BG_CALLER else None
        L.check(L.lib().pnr_ray_batch(
            L.ptr(self.images), int(self.images.dtype == torch.uint8), L.ptr(self.cams), self.F, self.h, self.w,
            L.ptr(state), frame_i, L.ptr(frame_dev), code, S, self.dir_norm, self.bg_mode, L.ptr(out["raydir"]),
            L.ptr(out["pixel_idx"]), L.ptr(out["gt_image"]), L.ptr(out["campos"]), L.ptr(out["camrotc2w"]),
            L.ptr(bg), L.ptr(out["id"]), L.stream_ptr(self.device)), "pnr_ray_batch")
        if self.intrinsics.shape[0] > 1:
            torch.index_select(self.intrinsics, 0, out["id"], out=out["intrinsic"])
        else:
            out["intrinsic"] = self.intrinsics
        if self.bg_mode == BG_CALLER:
            out["bg_color"] = self.bg_tensor.reshape(1, -1)
        out.update(near=self.near, far=self.far, h=self.h, w=self.w)
        return out

    def sample(self, size=None, mode: str = "random", frame=None, out: dict | None = None) -> dict:
        """The next training batch as the reference's item, on the device:
        campos [1,3], camrotc2w [1,3,3], raydir [1,R,3], pixel_idx [1,R,2],
        gt_image [1,R,3], bg_color [1,C], id [1] int32, intrinsic, and the host
        scalars near, far, h, w; R = size^2 ('random': independent pixels with
        replacement; 'patch': a size x size window) or h * w ('full').  So
        ``model(**item)`` and ``RenderLoss(opt)(out, item["gt_image"], model=model)``
        run as they are.

        frame: an int (the caller's epoch order), a device int32 tensor of one
        element (say one entry of a device randperm), or None: drawn on the
        device.  out: a previous item of the same size, overwritten in place.
        The step counter advances by one on the device."""
        code = mode_code(mode)
        S, R = self._rays(code, size)
        return self._batch(self._state, code, S, R, frame, out)

    def frame(self, i: int, out: dict | None = None) -> dict:
        """The full-frame item of image i (evaluation).  The training counter
        does not move; a 'random' background draws frame i's own coin."""
        self._eval_state[1] = int(i)
        return self._batch(self._eval_state, RAYS_FULL, 0, self.h * self.w, int(i), out)

    def probe_frames(self, ids):
        """The dicts ``probe_hole`` takes, one full frame per id."""
        for i in ids:
            it = self.frame(i)
            yield dict(campos=it["campos"], camrotc2w=it["camrotc2w"], raydir=it["raydir"][0],
                       gt_image=it["gt_image"][0], bg_color=it["bg_color"], pixel_idx=None, h=self.h, w=self.w,
                       near=self.near, far=self.far)
