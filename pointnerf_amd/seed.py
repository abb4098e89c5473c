"""Neural points from a raw cloud and the posed images of a ``FrameSet``.

``seed_points`` is the geometric part of the reference's initialisation
(run/train_ft.py:678-740, the ``load_points`` path): the ``ranges`` box, the
visual-hull carve of mvs_utils.alpha_masking (models/mvs/mvs_utils.py:573-607),
the optional voxel down-sampling, nearest_view (train_ft.py:42-51) and the
per-view colour / direction lookup of query_embedding(pointdir_w=True).  Its
result is the arguments of ``NeuralPoints.set_points``.  The MVSNet networks
(depth estimation, image features) stay out of scope.

Three HIP kernels (csrc/seed.hip): pnr_alpha_bits packs the alpha masks into
bit planes once, pnr_seed_mask votes and compacts, pnr_seed_view picks each
survivor's view and samples it.  One host read: the survivor count.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .rays import FrameSet, _tensor
from .voxelize import construct_vox_points_closest

CAM_TILE = L.SEED_CAM_TILE
EMBEDDING_CHANNELS = 32   # point_features_dim of the reference's checkpoints


def alpha_bits(alphas, frames: FrameSet) -> torch.Tensor:
    """Bit planes [F,H,ceil(W/32)] int32 of ``alphas > 0.1``: [F,H,W] float,
    bool, or uint8 (read as / 255), numpy or torch."""
    a = _tensor(alphas)
    if tuple(a.shape) != (frames.F, frames.h, frames.w):
        raise L.PnrError(f"alphas must be [F,H,W] = {(frames.F, frames.h, frames.w)}, got {tuple(a.shape)}")
    if a.dtype != torch.uint8:
        if not (a.dtype.is_floating_point or a.dtype == torch.bool):
            raise L.PnrError(f"alphas must be uint8, bool or float, got {a.dtype}")
        a = a.float()
    a = a.to(frames.device).contiguous()
    pitch = (frames.w + 31) // 32
    bits = torch.empty((frames.F, frames.h, pitch), dtype=torch.int32, device=frames.device)
    L.check(L.lib().pnr_alpha_bits(L.ptr(a), int(a.dtype == torch.uint8), frames.F, frames.h, frames.w, L.ptr(bits),
                                   pitch, bits.numel(), L.stream_ptr(frames.device)), "pnr_alpha_bits")
    return bits


def _host_floats(v, n: int, name: str):
    if v is None:
        return None
    vals = [float(x) for x in _tensor(v).reshape(-1).tolist()]
    if len(vals) != n:
        raise L.PnrError(f"{name}: {n} values, got {len(vals)}")
    return (L.c_float * n)(*vals)


def seed_mask(xyz: torch.Tensor, frames: FrameSet, bits=None, ranges=None, near_far=None, inall_img=1):
    """src_idx [M] int64: the points of xyz [N,3] (device, fp32) that pass the
    box and every view, in input order."""
    n = xyz.shape[0]
    dev = xyz.device
    scratch = L.scratch("pnr_seed_scratch_bytes", n, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().pnr_seed_mask(L.ptr(xyz), n, L.ptr(frames.cams), frames.F, frames.h, frames.w, L.ptr(bits),
                                  (frames.w + 31) // 32, _host_floats(ranges, 6, "ranges"),
                                  _host_floats(near_far, 2, "near_far"), int(inall_img), L.ptr(keep), L.ptr(src), n,
                                  L.ptr(count), L.ptr(scratch), scratch.numel(), L.stream_ptr(dev)), "pnr_seed_mask")
    m = int(count.item())   # the one host read
    return src[:m].long()


def seed_view(xyz: torch.Tensor, frames: FrameSet):
    """(cam_ind [M] int32, dirs [M,3], color [M,3], in_view [M] bool) of the
    points xyz [M,3] (device, fp32): each point's nearest view, its unit
    direction from that camera and the image's bilinear sample there."""
    m = xyz.shape[0]
    dev = xyz.device
    cam_ind = torch.empty(m, dtype=torch.int32, device=dev)
    dirs = torch.empty((m, 3), dtype=torch.float32, device=dev)
    color = torch.empty((m, 3), dtype=torch.float32, device=dev)
    in_view = torch.empty(m, dtype=torch.uint8, device=dev)
    L.check(L.lib().pnr_seed_view(L.ptr(xyz), m, L.ptr(frames.images), int(frames.images.dtype == torch.uint8),
                                  L.ptr(frames.cams), frames.F, frames.h, frames.w, L.ptr(cam_ind), L.ptr(dirs),
                                  L.ptr(color), L.ptr(in_view), m, L.stream_ptr(dev)), "pnr_seed_view")
    return cam_ind, dirs, color, in_view.bool()


def seed_points(xyz, frames: FrameSet, alphas=None, ranges=None, near_far=None, inall_img=1, vox_res=0,
                default_conf=-1.0, embedding="randn", seed=0) -> dict:
    """xyz [N,3] (numpy or torch) and the posed images of ``frames`` ->
    dict(xyz [M,3], embedding [1,M,32], color [1,M,3], dirs [1,M,3], conf
    [1,M,1], cam_ind [M] int32, src_idx [M] int64, in_view [M] bool) on the
    frames' device.  ``NeuralPoints(opt, dev, **{k: out[k] for k in ("xyz",
    "embedding", "color", "dirs", "conf")})`` takes it as it stands.

    alphas [F,H,W]: the views' silhouettes (> 0.1 is inside) for the hull
    carve, or None.  ranges: (lo xyz, hi xyz), a closed box; None or ranges[0]
    <= -99 disables it.  near_far = (n, f): every view also asks n - 1 <= cz <=
    f.  inall_img: 1 tests a point that projects outside a view against that
    view's border pixel (behind the camera: carved), 0 lets it pass the view.
    vox_res > 0 keeps the point closest to the centroid of each voxel of a
    vox_res^3 grid over the survivors.  conf is 1, or default_conf when 0 <
    default_conf <= 1.  embedding: 'randn' (torch.Generator(seed)) or 'zeros'.
    src_idx indexes the caller's xyz."""
    if not isinstance(frames, FrameSet):
        raise L.PnrError("seed_points: frames must be a FrameSet")
    if embedding not in ("randn", "zeros"):
        raise L.PnrError(f"embedding '{embedding}': 'randn' or 'zeros'")
    dev = frames.device
    pts = _tensor(xyz)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise L.PnrError(f"xyz must be [N,3] with N >= 1, got {tuple(pts.shape)}")
    pts = pts.detach().to(dev).float().contiguous()
    bits = alpha_bits(alphas, frames) if alphas is not None else None
    src_idx = seed_mask(pts, frames, bits, ranges, near_far, inall_img)
    if int(vox_res) > 0 and src_idx.numel() > 0:
        _, _, min_idx = construct_vox_points_closest(pts.index_select(0, src_idx), int(vox_res))
        src_idx = src_idx.index_select(0, min_idx)
    out_xyz = pts.index_select(0, src_idx)
    m = out_xyz.shape[0]
    cam_ind, dirs, color, in_view = seed_view(out_xyz, frames)
    conf_val = float(default_conf) if 0.0 < float(default_conf) <= 1.0 else 1.0   # neural_points.py:483
    if embedding == "randn":
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        emb = torch.randn((1, m, EMBEDDING_CHANNELS), generator=gen, dtype=torch.float32, device=dev)
    else:
        emb = torch.zeros((1, m, EMBEDDING_CHANNELS), dtype=torch.float32, device=dev)
    return dict(xyz=out_xyz, embedding=emb, color=color[None], dirs=dirs[None],
                conf=torch.full((1, m, 1), conf_val, dtype=torch.float32, device=dev), cam_ind=cam_ind,
                src_idx=src_idx, in_view=in_view)
