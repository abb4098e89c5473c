"""Dev tool: time fuse_depth_maps on a synthetic scene, a sphere
of radius 1 over the plane z = -1 with analytic depths seen from the headline
bench's camera ring (F views of size x size), next to a plain torch
restatement of the reference's per-pair loop on the same GPU
(reproject_with_depth_gpu / check_geometric_consistency_gpu / the sums of
filter_by_masks_gpu, models/mvs/filter_utils.py:157-264: two 4x4 inversions and
about thirty [H,W] or [3,HW] temporaries per pair, grid_sample with
align_corners=True).  Prints one JSON line: median ms of the whole call, of
each entry point, and of the restatement."""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pointnerf_amd import _lib as L  # noqa: E402
from pointnerf_amd import fuse as FU  # noqa: E402
from pointnerf_amd import synthetic as S  # noqa: E402
from pointnerf_amd.rays import FrameSet  # noqa: E402


def timed(fn, warmup, repeats):
    """(median, min, max) ms of fn() by HIP events, after ``warmup`` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return round(times[len(times) // 2], 3), round(times[0], 3), round(times[-1], 3)


def analytic_depths(campos, camrot, K, H, W, radius=1.0, plane=-1.0, far=12.0):
    """[F,H,W] fp32 camera-space z of the first hit of each pixel-centre ray
    with the sphere at the origin or the plane; 0 where nothing is hit."""
    dev = campos.device
    jj, ii = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    dc = torch.stack([(ii + 0.5 - K[0, 2]) / K[0, 0], (jj + 0.5 - K[1, 2]) / K[1, 1], torch.ones_like(ii) * 1.0], -1)
    out = []
    for f in range(campos.shape[0]):
        dw = dc.double() @ camrot[f].double().t()
        o = campos[f].double()
        tp = (plane - o[2]) / dw[..., 2]
        t = torch.where(tp > 0, tp, torch.full_like(tp, float("inf")))
        a, b, c = (dw * dw).sum(-1), 2 * (dw @ o), o @ o - radius ** 2
        disc = b * b - 4 * a * c
        ts = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
        t = torch.where((disc >= 0) & (ts > 0) & (ts < t), ts, t)
        out.append(torch.where(t <= far, t, torch.zeros_like(t)).float())
    return torch.stack(out)


# ------------------------------------------------- the reference's formulation
def _lift(K, px, depth):
    """[3,HW] camera points of homogeneous pixels px [3,HW] at depth [HW]."""
    return torch.linalg.inv(K) @ (px * depth)


def _move(E_to, E_from, pts):
    """[3,HW] points carried from one camera to another through 4x4 world-to-camera matrices."""
    ones = torch.ones_like(pts[:1])
    return ((E_to @ torch.linalg.inv(E_from)) @ torch.cat([pts, ones], 0))[:3]


def _pixels(K, pts):
    q = K @ pts
    return q[:2] / q[2:3]


def torch_pair(d_ref, d_src, K, E_ref, E_src, grid_px):
    """One (reference, source) pair as the reference computes it: lift, move,
    project, sample the source depth (align_corners=True, border padding),
    lift, move back, project.  Returns (depth, x, y) reprojected, [H,W] each."""
    H, W = d_ref.shape
    in_src = _move(E_src, E_ref, _lift(K, grid_px, d_ref.reshape(-1)))
    uv = _pixels(K, in_src)
    us, vs = uv[0].reshape(H, W).float(), uv[1].reshape(H, W).float()
    outside = (us >= W) | (us < 0) | (vs >= H) | (vs < 0)   # the reference's vis_mask, summed there too
    norm = torch.stack([us * 2 / (W - 1) - 1, vs * 2 / (H - 1) - 1], -1)[None]
    d_s = Fn.grid_sample(d_src[None, None], norm, mode="bilinear", padding_mode="border", align_corners=True)
    back = _move(E_ref, E_src, _lift(K, torch.cat([uv, torch.ones_like(uv[:1])], 0), d_s.reshape(-1)))
    uv2 = _pixels(K, back)
    return back[2].reshape(H, W).float(), uv2[0].reshape(H, W).float(), uv2[1].reshape(H, W).float(), outside


def torch_filter(depths, K, w2c, geo_cnsst_num=3, views=None):
    """The pair loop and the sums of the reference's filter for the reference
    views ``views`` (all by default); returns the survivor count."""
    F, H, W = depths.shape
    dev = depths.device
    gy, gx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    grid_px = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.ones(H * W, device=dev, dtype=gx.dtype)], 0)
    kept = 0
    for r in (range(F) if views is None else views):
        d_sum, n_match, n_vis = 0, 0, 0
        for s in range(F):
            if s == r:
                continue
            d2, x2, y2, outside = torch_pair(depths[r], depths[s], K, w2c[r], w2c[s], grid_px)
            dist = torch.sqrt((x2 - gx) ** 2 + (y2 - gy) ** 2)
            rel = torch.abs(d2 - depths[r]) / depths[r]
            ok = (dist < 1) & (rel < 0.01)
            d2[~ok] = 0
            n_vis = n_vis + (~outside).float()
            n_match = n_match + ok.to(torch.int32)
            d_sum = d_sum + d2
        avg = (d_sum + depths[r]) / (n_match + 1)
        final = (n_match >= geo_cnsst_num) & (depths[r] > 0)
        kept = kept + avg[final].numel()
    return kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-views", type=int, default=2,
                    help="reference views the torch restatement is timed on (scaled to all of them); 0: skip it")
    ap.add_argument("--torch-repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, W = a.views, a.size, a.size
    cams = [S.camera(360.0 * f / F, -30.0, 4.0) for f in range(F)]
    campos, camrot = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    focal = S.lego_focal(800) * H / 800.0
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]])
    fs = FrameSet(torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev), (campos, camrot), K, 2.0, 6.0, device=dev)
    pos_t, rot_t, Kt = torch.from_numpy(campos).to(dev), torch.from_numpy(camrot).to(dev), torch.from_numpy(K).to(dev)
    depths = analytic_depths(pos_t, rot_t, Kt, H, W)

    res = {"views": F, "size": H, "lib": os.path.basename(L.LIB_PATH)}
    out = FU.fuse_depth_maps(depths, fs, return_maps=True)
    valid = depths > 0
    res["valid_px"] = int(valid.sum())
    res["survivors"] = int(out["xyz"].shape[0])
    res["visible_pairs"] = int(out["visible_map"].sum())
    res["matches"] = int(out["count_map"].sum())

    # the entry points on their own, with preallocated outputs
    n = F * H * W
    scratch = L.scratch("pnr_depth_fuse_scratch_bytes", F, H, W, device=dev)
    keep, src = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    prm = FU.fuse_params()
    m = res["survivors"]
    xyz, conf = torch.empty((m, 3), device=dev), torch.empty(m, device=dev)
    spx, cnt = torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
    st = L.stream_ptr(dev)

    def run_fuse():
        L.check(L.lib().pnr_depth_fuse(L.ptr(depths), None, None, L.ptr(fs.cams), F, H, W, ctypes.byref(prm),
                                       L.ptr(out["depth_avg"]), L.ptr(out["count_map"]), L.ptr(out["visible_map"]),
                                       L.ptr(keep), L.ptr(src), n, L.ptr(total), L.ptr(scratch), scratch.numel(), st),
                "pnr_depth_fuse")

    def run_points():
        L.check(L.lib().pnr_depth_points(L.ptr(src), m, L.ptr(out["depth_avg"]), L.ptr(out["count_map"]), None,
                                         L.ptr(fs.cams), F, H, W, ctypes.byref(prm), L.ptr(xyz), L.ptr(conf),
                                         L.ptr(spx), L.ptr(cnt), m, st), "pnr_depth_points")

    res["hip_ms"] = {
        "fuse_depth_maps": timed(lambda: FU.fuse_depth_maps(depths, fs), a.warmup, a.repeats),
        "depth_fuse+compact": timed(run_fuse, a.warmup, a.repeats),
        "depth_points": timed(run_points, a.warmup, a.repeats),
    }
    pairs = res["valid_px"] * (F - 1)
    res["model"] = {"pair_tests_G": round(pairs / 1e9, 3), "sampled_pairs_G": round(res["visible_pairs"] / 1e9, 3),
                    "depth_MB": round(n * 4 / 1e6, 1), "written_MB": round(n * 16 / 1e6, 1),
                    "pair_tests_per_ns": round(pairs / 1e6 / res["hip_ms"]["depth_fuse+compact"][0], 2)}
    if a.torch_views > 0 and F > 1:
        c2w = torch.eye(4, device=dev, dtype=torch.float32).repeat(F, 1, 1)
        c2w[:, :3, :3], c2w[:, :3, 3] = rot_t, pos_t
        w2c = torch.inverse(c2w)
        views = list(range(0, F, max(F // a.torch_views, 1)))[:a.torch_views]
        med = timed(lambda: torch_filter(depths, Kt.float(), w2c, views=views), 1, a.torch_repeats)
        res["torch_ms"] = {"ref_views_timed": len(views), "per_ref_view": round(med[0] / len(views), 3),
                           "all_views": round(med[0] / len(views) * F, 1)}
        res["speedup"] = round(res["torch_ms"]["all_views"] / res["hip_ms"]["fuse_depth_maps"][0], 1)
    assert math.isfinite(res["hip_ms"]["fuse_depth_maps"][0])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
