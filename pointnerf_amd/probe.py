"""Point growing: which rays see a surface where no neural point is.

``probe_hole`` restates the frame loop of run/train_ft.py:420-533 and
``select_grow_candidates`` its per-frame selection (:496-508, bloat_inds
:535-543) in torch ops on [H,W,.] maps (not hot; any device).  The maps come
from ``NeuralPointsRayMarching.probe_rays`` -- the render plus the opt.prob == 1
outputs of neural_points_volumetric_model_ori.py:351-372, one pnr_probe launch
per ray chunk.  The result feeds ``checkpoint.grow_points``.
"""
from __future__ import annotations

import torch

from . import _lib as L

MAP_KEYS = ("coarse_raycolor", "ray_mask", "ray_max_sample_loc_w", "ray_max_far_dist", "ray_max_shading_opacity",
            "shading_avg_color", "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding")


def select_grow_candidates(maps, gt_image, bg, edge_mask=None, far_thresh=-1.0, opacity_thresh=0.7):
    """bool [H,W]: the pixels whose most opaque sample becomes a new point
    (train_ft.py:496-508).  maps: [H,W,.] tensors ray_mask,
    ray_max_shading_opacity and, with far_thresh > 0, ray_max_far_dist and
    coarse_raycolor; gt_image [H,W,C]; bg broadcastable to it; edge_mask
    [H,W] bool or None (every pixel was rendered).

    miss = ray_mask < 1 and |gt - bg| > 0.002 (inside edge_mask); its 3x3
    dilation, indices clamped at the border as bloat_inds does, or -- with
    far_thresh > 0 -- a hit ray whose nearest neighbour is farther than
    far_thresh while |gt - render| < 0.1; kept where ray_mask > 0 and the
    maximum opacity exceeds opacity_thresh."""
    H, W = gt_image.shape[:2]
    dev = gt_image.device
    ray_mask = maps["ray_mask"].reshape(H, W).float()
    miss = (ray_mask < 1) & (torch.norm(gt_image - bg, dim=-1) > 0.002)
    if edge_mask is not None:
        miss = miss & edge_mask.reshape(H, W).bool()
    d = torch.arange(-1, 2, device=dev)
    shift = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).reshape(1, 9, 2)
    nb = (miss.nonzero()[:, None, :] + shift).reshape(-1, 2)
    near = torch.zeros((H, W), dtype=torch.bool, device=dev)
    near[nb[:, 0].clamp(0, H - 1), nb[:, 1].clamp(0, W - 1)] = True
    if far_thresh > 0:
        render = maps["coarse_raycolor"].reshape(H, W, -1)
        if render.shape[-1] != gt_image.shape[-1]:
            raise L.PnrError(f"far_thresh > 0 compares gt_image ({gt_image.shape[-1]} channels) with "
                             f"coarse_raycolor ({render.shape[-1]} channels)")
        near = near | ((ray_mask > 0) & (maps["ray_max_far_dist"].reshape(H, W) > far_thresh)
                       & (torch.norm(gt_image - render, dim=-1) < 0.1))
    return (ray_mask > 0) & near & (maps["ray_max_shading_opacity"].reshape(H, W) > opacity_thresh)


def frame_maps(out, pixel_idx, h, w):
    """Scatter a ray batch's outputs [1,R,C] into [h,w,C] maps (train_ft.py:485-494)
    and the rendered-pixel mask [h,w] (:467-469).  pixel_idx [...,2] = (x, y)
    per ray, or None = the whole frame in row-major order."""
    dev = out["ray_mask"].device
    if pixel_idx is None:
        flat = torch.arange(h * w, device=dev)
    else:
        px = pixel_idx.reshape(-1, 2).to(dev).long()
        flat = px[:, 1] * w + px[:, 0]
    edge = torch.zeros(h * w, dtype=torch.bool, device=dev)
    edge[flat] = True
    maps = {}
    for k in MAP_KEYS:
        v = out[k]
        if v is None:
            maps[k] = None
            continue
        v = v.reshape(flat.numel(), -1)
        m = torch.zeros((h * w, v.shape[-1]), dtype=v.dtype, device=dev)
        m[flat] = v
        maps[k] = m.reshape(h, w, -1)
    return maps, edge.reshape(h, w), flat


def probe_hole(model, frames, opt, opacity_thresh=0.7, test_steps=0, compound_prob_mul=True):
    """(add_xyz [M,3], add_embedding [M,32], add_color, add_dir, add_conf) for
    ``checkpoint.grow_points`` (None for a table the cloud lacks): the frame
    loop of train_ft.py:459-515.

    frames: iterable of dicts campos, camrotc2w, raydir [R,3], gt_image [R,C]
    (the rendered pixels' ground truth, in ray order), bg_color, pixel_idx
    ([R,2] (x, y)) or None, h, w; optional near / far (default opt.near_plane /
    far_plane).  Each frame is rendered by ``model.probe_rays`` with
    model.opt.prob = 1 and, when opt.prob_kernel_size is set, model.opt.query_size
    = the tier of test_steps (:428-432); both are restored on return.

    compound_prob_mul=True reproduces :512 -- the *accumulated* add_conf is
    multiplied by opt.prob_mul after every frame, so the points of frame i of n
    end at conf * prob_mul^(n - i); False multiplies each point's conf once."""
    mopt = model.opt
    saved = (getattr(mopt, "prob", 0), getattr(mopt, "query_size", None))
    far_thresh = float(getattr(opt, "far_thresh", -1.0))
    prob_mul = float(getattr(opt, "prob_mul", 1.0))
    names = ("ray_max_sample_loc_w", "shading_avg_embedding", "shading_avg_color", "shading_avg_dir",
             "shading_avg_conf")
    acc = None
    try:
        pks = getattr(opt, "prob_kernel_size", None)
        if pks is not None:
            tier = sum(1 for t in getattr(opt, "prob_tiers", ()) if t < test_steps)
            mopt.query_size = [int(x) for x in list(pks)[tier * 3:tier * 3 + 3]]
        mopt.prob = 1
        for fr in frames:
            h, w = int(fr["h"]), int(fr["w"])
            out = model.probe_rays(fr["campos"], fr["camrotc2w"], fr["raydir"],
                                   float(fr.get("near", getattr(opt, "near_plane", 0.0))),
                                   float(fr.get("far", getattr(opt, "far_plane", 0.0))), fr["bg_color"])
            maps, edge, flat = frame_maps(out, fr.get("pixel_idx"), h, w)
            dev = edge.device
            gt_rows = fr["gt_image"].to(dev).float().reshape(flat.numel(), -1)
            gt = torch.zeros((h * w, gt_rows.shape[-1]), dtype=torch.float32, device=dev)
            gt[flat] = gt_rows
            sel = select_grow_candidates(maps, gt.reshape(h, w, -1), fr["bg_color"].to(dev).float().reshape(-1),
                                         edge, far_thresh, opacity_thresh)
            new = [None if maps[k] is None else maps[k][sel] for k in names]
            if acc is None:
                acc = new
            else:
                acc = [None if (a is None or n is None) else torch.cat([a, n], 0) for a, n in zip(acc, new)]
            if acc[4] is not None:
                if compound_prob_mul:
                    acc[4] = acc[4] * prob_mul
                else:
                    acc[4][acc[4].shape[0] - new[4].shape[0]:] *= prob_mul
    finally:
        mopt.prob = saved[0]
        if saved[1] is not None:
            mopt.query_size = saved[1]
    if acc is None:   # no frames
        dev = getattr(getattr(model, "neural_points", None), "device", "cpu")
        acc = [torch.zeros((0, c), device=dev) for c in (3, 32, 3, 3, 1)]
    return tuple(acc)
