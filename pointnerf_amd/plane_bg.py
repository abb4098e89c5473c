"""The per-ray background of the reference's ``bgmodel="plane"``.

With that flag (all of dev_scripts/dtu_test_inf/*.sh) the reference does not
composite over a constant colour: it intersects every ray with the table plane
(mvs_utils.gen_bg_points / get_rayplane_cross, models/mvs/mvs_utils.py:380-408),
looks the point up in every source image, keeps the samples that look like the
plane and that no neural point covers (set_bg,
models/mvs_points_volumetric_model.py:279-317; homo_warp_fg_mask,
mvs_utils.py:318-331), takes their per-channel maximum as ``bg_ray`` and adds
``coarse_is_background * bg_ray`` to the rendered colour (fill_invalid,
models/neural_points_volumetric_model_ori.py:109-111).

``PlaneBackground`` does this on the images and cameras a ``FrameSet`` already
holds on the device, with two HIP kernels (csrc/plane_bg.hip):
pnr_plane_fg_masks marks the pixels the cloud covers in every view, once per
cloud; pnr_plane_bg makes ``bg_ray`` for a ray batch in one launch and, in its
fused form, finishes the frame.  Evaluation only.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .rays import FrameSet, _tensor, camera_rays

CAM_TILE = L.PLANE_CAM_TILE
FIT_THRESH = 0.03      # set_bg's thresh, mvs_points_volumetric_model.py:311
DOT_EPSILON = 1e-3     # get_rayplane_cross's epsilon, mvs_utils.py:387


def _host3(v, name: str):
    vals = [float(x) for x in _tensor(v).detach().reshape(-1).tolist()]
    if len(vals) != 3:
        raise L.PnrError(f"{name}: 3 values, got {len(vals)}")
    return (L.c_float * 3)(*vals)


class PlaneBackground:
    """``bg_ray`` of the plane (plane_pnt, plane_normal: host values, the normal
    not normalised; plane_color in [0, 1]) seen through the source views of
    ``frames``.  Give the cloud (points_xyz [N,3], e.g.
    ``model.neural_points.xyz``; N = 0 is an empty cloud) or the masks
    themselves (fg_masks [F,H,W] uint8 / bool: nonzero = covered)."""

    def __init__(self, frames: FrameSet, plane_pnt, plane_normal, plane_color, points_xyz=None, fg_masks=None):
        if not isinstance(frames, FrameSet):
            raise L.PnrError("PlaneBackground: frames must be a FrameSet")
        if (points_xyz is None) == (fg_masks is None):
            raise L.PnrError("PlaneBackground: give points_xyz or fg_masks (one of them)")
        self.frames = frames
        self.device = frames.device
        self.plane_pnt, self.plane_normal = _tensor(plane_pnt).detach().cpu(), _tensor(plane_normal).detach().cpu()
        self._pnt = _host3(plane_pnt, "plane_pnt")
        self._normal = _host3(plane_normal, "plane_normal")
        self._color = _host3(plane_color, "plane_color")
        if fg_masks is not None:
            m = _tensor(fg_masks)
            shape = (frames.F, frames.h, frames.w)
            if tuple(m.shape) != shape:
                raise L.PnrError(f"fg_masks must be [F,H,W] = {shape}, got {tuple(m.shape)}")
            if m.dtype not in (torch.uint8, torch.bool):
                raise L.PnrError(f"fg_masks must be uint8 or bool, got {m.dtype}")
            self.fg_masks = m.to(self.device).to(torch.uint8).contiguous()
        else:
            self.fg_masks = torch.empty((frames.F, frames.h, frames.w), dtype=torch.uint8, device=self.device)
            self.refresh_fg(points_xyz)

    # ------------------------------------------------------------------ masks
    def refresh_fg(self, points_xyz) -> torch.Tensor:
        """Rebuild the foreground masks from the cloud (after prune or grow):
        fg_masks [F,H,W] uint8, in place."""
        pts = _tensor(points_xyz)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise L.PnrError(f"points_xyz must be [N,3], got {tuple(pts.shape)}")
        pts = pts.detach().to(self.device).float().contiguous()
        fs = self.frames
        self.fg_masks.zero_()
        L.check(L.lib().pnr_plane_fg_masks(L.ptr(pts), pts.shape[0], L.ptr(fs.cams), fs.F, fs.h, fs.w,
                                           L.ptr(self.fg_masks), self.fg_masks.numel(), L.stream_ptr(self.device)),
                "pnr_plane_fg_masks")
        return self.fg_masks

    # ------------------------------------------------------------------- rays
    def _ray_args(self, campos, raydir):
        c = _tensor(campos)
        if c.numel() != 3:
            raise L.PnrError(f"campos must be [1,3] (one camera), got {tuple(c.shape)}")
        d = _tensor(raydir)
        if d.dim() not in (2, 3) or d.shape[-1] != 3 or (d.dim() == 3 and d.shape[0] != 1):
            raise L.PnrError(f"raydir must be [1,R,3] or [R,3], got {tuple(d.shape)}")
        c = c.detach().to(self.device).float().reshape(3).contiguous()
        d = d.detach().to(self.device).float().reshape(-1, 3).contiguous()
        return c, d

    def _launch(self, c, d, bg, is_bg=None, ray_color=None):
        fs = self.frames
        L.check(L.lib().pnr_plane_bg(L.ptr(c), L.ptr(d), d.shape[0], L.ptr(fs.images),
                                     int(fs.images.dtype == torch.uint8), L.ptr(fs.cams), fs.F, fs.h, fs.w,
                                     L.ptr(self.fg_masks), self.fg_masks.numel(), self._pnt, self._normal,
                                     self._color, L.ptr(bg), bg.shape[0], L.ptr(is_bg), L.ptr(ray_color),
                                     L.stream_ptr(self.device)), "pnr_plane_bg")

    def rays(self, campos, raydir) -> torch.Tensor:
        """bg_ray [1,R,3] of the rays raydir [1,R,3] (or [R,3]) from campos
        [1,3]: gen_bg_points + set_bg, one launch."""
        c, d = self._ray_args(campos, raydir)
        bg = torch.empty((d.shape[0], 3), dtype=torch.float32, device=self.device)
        self._launch(c, d, bg)
        return bg[None]

    def _check_color(self, who: str, color, is_bg, R: int):
        if not torch.is_tensor(color) or color.shape[-1] != 3:
            ch = color.shape[-1] if torch.is_tensor(color) else "no"
            raise L.PnrError(f"{who}: the colour has {ch} channels, the plane background 3 "
                             "(a 128-channel 'cnn' render has no plane background)")
        if color.requires_grad or (torch.is_tensor(is_bg) and is_bg.requires_grad):
            raise L.PnrError(f"{who}: the colour requires grad; the plane background is evaluation only: "
                             "pnr_composite_bwd propagates no is_bg gradient, so a training step would silently "
                             "lose the d colour / d T_bg term")
        L.require_gpu(color)
        if color.dtype != torch.float32 or color.numel() != R * 3:
            raise L.PnrError(f"{who}: colour must be fp32 [1,{R},3], got {color.dtype} {tuple(color.shape)}")
        if not torch.is_tensor(is_bg) or is_bg.numel() != R:
            got = tuple(is_bg.shape) if torch.is_tensor(is_bg) else type(is_bg).__name__
            raise L.PnrError(f"{who}: is_bg must be [1,{R},1], got {got}")

    def fill(self, out: dict, bg_ray: torch.Tensor) -> dict:
        """fill_invalid on a forward's output rendered with ``bg_ray=``:
        coarse_raycolor = coarse_raycolor + coarse_is_background * bg_ray (a new
        tensor; the dict is returned)."""
        color, is_bg = out["coarse_raycolor"], out["coarse_is_background"]
        R = bg_ray.numel() // 3
        self._check_color("fill", color, is_bg, R)
        out["coarse_raycolor"] = color + is_bg.to(color.dtype).reshape(1, R, 1) * bg_ray.reshape(1, R, 3)
        return out

    def fused(self, campos, raydir, is_bg: torch.Tensor, ray_color: torch.Tensor) -> torch.Tensor:
        """rays + fill in one launch: returns bg_ray [1,R,3] and adds is_bg *
        bg_ray to ray_color [1,R,3] (fp32, contiguous) in place."""
        c, d = self._ray_args(campos, raydir)
        R = d.shape[0]
        self._check_color("fused", ray_color, is_bg, R)
        if not ray_color.is_contiguous():
            raise L.PnrError("fused: ray_color must be contiguous (it is updated in place)")
        w = is_bg.detach().to(self.device).float().reshape(R).contiguous()
        bg = torch.empty((R, 3), dtype=torch.float32, device=self.device)
        self._launch(c, d, bg, w, ray_color)
        return bg[None]

    def frame(self, campos, camrotc2w, intrinsic, h: int, w: int) -> torch.Tensor:
        """bg_ray [1,h,w,3] of a whole view (create_all_bg's per-view map,
        run/train_ft.py:552-579), its rays from camera_rays."""
        rot = _tensor(camrotc2w).reshape(3, 3)
        raydir = camera_rays(intrinsic, rot, int(h), int(w), device=self.device)
        return self.rays(campos, raydir).reshape(1, int(h), int(w), 3)

    # ------------------------------------------------------------------ plane
    def near_plane(self, xyz: torch.Tensor, thresh: float = 0.2) -> torch.Tensor:
        """dataset.filter_plane (data/dtu_ft_dataset.py:927-934): True for the
        points within ``thresh`` of the plane, |n . x + d| < thresh with the
        normal as given.  Torch ops on xyz's device."""
        n = self.plane_normal.to(xyz.device, xyz.dtype).reshape(3)
        p = self.plane_pnt.to(xyz.device, xyz.dtype).reshape(3)
        a, b, c = n[0], n[1], n[2]
        d = -a * p[0] - b * p[1] - c * p[2]
        return torch.abs(xyz[..., 0] * a + xyz[..., 1] * b + xyz[..., 2] * c + d) < thresh
