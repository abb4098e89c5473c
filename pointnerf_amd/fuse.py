"""A seed cloud from posed depth maps.

``fuse_depth_maps`` is the geometric filter of the reference's ``gen_points``
(filter_by_masks_gpu, models/mvs/filter_utils.py:157-291): every valid pixel
of every view is projected into every other view and brought back through that
view's depth; a pixel is kept when enough views agree, and the agreeing depths
are averaged.  The depth maps may come from anywhere: an MVS dump, sensor
depth, lidar depth rendered per camera.  Its ``xyz`` is the raw cloud that
``seed_points`` takes.  The MVSNet networks stay out of scope.

Two HIP kernels (csrc/fuse.hip): pnr_depth_fuse tests every pair in one pass
and compacts, pnr_depth_points writes the survivors.  One host read: the
survivor count.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .rays import FrameSet, _tensor


def _map(a, frames: FrameSet, name: str, as_mask: bool = False) -> torch.Tensor:
    t = _tensor(a).detach()
    if tuple(t.shape) != (frames.F, frames.h, frames.w):
        raise L.PnrError(f"{name} must be [F,H,W] = {(frames.F, frames.h, frames.w)}, got {tuple(t.shape)}")
    if as_mask:
        if t.dtype not in (torch.uint8, torch.bool):
            raise L.PnrError(f"{name} must be uint8 or bool, got {t.dtype}")
        return t.to(frames.device).to(torch.uint8).contiguous()
    if not t.dtype.is_floating_point:
        raise L.PnrError(f"{name} must be float, got {t.dtype}")
    return t.to(frames.device).float().contiguous()


def fuse_params(geo_cnsst_num=3, conf_thresh=0.0, pix_thresh=1.0, rel_thresh=0.01, ranges=None,
                reassign_conf=False) -> L.FuseParams:
    """pnr_fuse_params; ranges None switches the box off (ranges[0] <= -99)."""
    box = [-100.0] * 6 if ranges is None else [float(x) for x in _tensor(ranges).reshape(-1).tolist()]
    if len(box) != 6:
        raise L.PnrError(f"ranges: 6 values, got {len(box)}")
    return L.FuseParams(float(pix_thresh), float(rel_thresh), float(conf_thresh), int(geo_cnsst_num),
                        int(bool(reassign_conf)), (L.c_float * 6)(*box))


def fuse_depth_maps(depths, frames: FrameSet, conf=None, mask=None, geo_cnsst_num=3, conf_thresh=0.0,
                    pix_thresh=1.0, rel_thresh=0.01, ranges=None, reassign_conf=False, return_maps=False) -> dict:
    """depths [F,H,W] (numpy or torch; depth = the camera-space z of
    ``frames``' cameras, <= 0 or non-finite: no measurement) -> dict(xyz [M,3]
    world points, conf [M], src_pixel [M] int64 flat index into [F,H,W], count
    [M] int32 agreeing views) on the frames' device, in ascending src_pixel.
    ``seed_points(out["xyz"], frames, ...)`` takes the cloud as it stands.

    A pixel is kept when at least geo_cnsst_num other views reproject onto it
    within pix_thresh pixels and rel_thresh relative depth (not asked of a
    single view), conf [F,H,W] > conf_thresh and mask [F,H,W] (uint8 or bool)
    != 0 where given, and its point, at the average of its own and the
    agreeing depths, lies in the closed box ranges = (lo xyz, hi xyz); None or
    ranges[0] <= -99 disables the box.  conf is the input confidence, or 1;
    with reassign_conf it is scaled by 1 - 1 / 1.14869^clamp(count -
    geo_cnsst_num + 1, 1, 10), the reference's default_conf > 1 branch.
    return_maps adds depth_avg [F,H,W] fp32, count_map and visible_map [F,H,W]
    int32 (0 on invalid pixels).  The exact rule is in include/pnr.h.

    Not built: the reference's far_plane_shift background points and its
    manual_depth_view branch."""
    if not isinstance(frames, FrameSet):
        raise L.PnrError("fuse_depth_maps: frames must be a FrameSet")
    dev = frames.device
    d = _map(depths, frames, "depths")
    c = _map(conf, frames, "conf") if conf is not None else None
    k = _map(mask, frames, "mask", as_mask=True) if mask is not None else None
    prm = fuse_params(geo_cnsst_num, conf_thresh, pix_thresh, rel_thresh, ranges, reassign_conf)
    F, H, W = frames.F, frames.h, frames.w
    n = F * H * W
    scratch = L.scratch("pnr_depth_fuse_scratch_bytes", F, H, W, device=dev)
    depth_avg = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    count_map, visible_map = (torch.empty((F, H, W), dtype=torch.int32, device=dev) for _ in range(2))
    keep, src = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    st = L.stream_ptr(dev)
    L.check(L.lib().pnr_depth_fuse(L.ptr(d), L.ptr(c), L.ptr(k), L.ptr(frames.cams), F, H, W, ctypes.byref(prm),
                                   L.ptr(depth_avg), L.ptr(count_map), L.ptr(visible_map), L.ptr(keep), L.ptr(src), n,
                                   L.ptr(total), L.ptr(scratch), scratch.numel(), st), "pnr_depth_fuse")
    m = int(total.item())   # the one host read
    xyz = torch.empty((m, 3), dtype=torch.float32, device=dev)
    conf_out = torch.empty(m, dtype=torch.float32, device=dev)
    src_pixel = torch.empty(m, dtype=torch.int64, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    L.check(L.lib().pnr_depth_points(L.ptr(src), m, L.ptr(depth_avg), L.ptr(count_map), L.ptr(c), L.ptr(frames.cams),
                                     F, H, W, ctypes.byref(prm), L.ptr(xyz), L.ptr(conf_out), L.ptr(src_pixel),
                                     L.ptr(count), m, st), "pnr_depth_points")
    out = dict(xyz=xyz, conf=conf_out, src_pixel=src_pixel, count=count)
    if return_maps:
        out.update(depth_avg=depth_avg, count_map=count_map, visible_map=visible_map)
    return out
