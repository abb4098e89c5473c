"""Dev tool: time seed_points on the headline bench's 2 M-point
synthetic cloud against F = 100 views of 800 x 800 with a disc silhouette, next
to a plain torch restatement of the reference's formulation on the same GPU:
the per-view loop of mvs_utils.alpha_masking (models/mvs/mvs_utils.py:573-607)
and nearest_view in 10 000-point slabs (run/train_ft.py:42-51), plus a
vectorised bilinear lookup.  Prints one JSON line: median ms of the whole call,
of each stage, and of the restatement's stages."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pointnerf_amd import seed as SD  # noqa: E402
from pointnerf_amd import synthetic as S  # noqa: E402
from pointnerf_amd.rays import FrameSet  # noqa: E402


def timed(fn, warmup, repeats):
    """Median ms of fn() by HIP events, after ``warmup`` untimed calls."""
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
    return sorted(times)[len(times) // 2]


# ------------------------------------------------- the reference's formulation
def torch_alpha_masking(points, alphas, intrinsic, w2cs):
    """alpha_masking with opt = None (inall_img = 1, no near_far): one pass over
    all N points per view."""
    w_xyz1 = torch.cat([points, torch.ones_like(points[:, :1])], -1)
    H, W = alphas.shape[1:]
    hull = None
    for i in range(alphas.shape[0]):
        cam_xyz = (w_xyz1 @ w2cs[i].t())[:, :3] @ intrinsic.t()
        img_xy = torch.floor(cam_xyz[:, :2] / cam_xyz[:, -1:] + 0.0).long()
        img_xy[:, 0] = torch.clamp(img_xy[:, 0], min=0, max=W - 1)
        img_xy[:, 1] = torch.clamp(img_xy[:, 1], min=0, max=H - 1)
        m = alphas[i][img_xy[:, 1], img_xy[:, 0]] > 0.1
        hull = m if hull is None else hull * m
    return hull > 0


def torch_nearest_view(campos, raydir, xyz, step=10000):
    cam_ind = torch.zeros([0, 1], device=campos.device, dtype=torch.long)
    for i in range(0, len(xyz), step):
        dists = xyz[i:min(len(xyz), i + step), None, :] - campos[None, ...]
        dists_norm = torch.norm(dists, dim=-1)
        dists_dir = dists / (dists_norm[..., None] + 1e-6)
        dists = dists_norm / 200 + (1.1 - torch.sum(dists_dir * raydir[None, :], dim=-1))
        cam_ind = torch.cat([cam_ind, torch.argmin(dists, dim=1).view(-1, 1)], dim=0)
    return cam_ind[:, 0]


def torch_lookup(xyz, cam_ind, images, campos, camrot, K):
    """dirs and the bilinear colour of each point in its view (texel centres at + 0.5)."""
    F, H, W, _ = images.shape
    d = xyz - campos[cam_ind]
    dirs = d / (torch.norm(d, dim=-1, keepdim=True) + 1e-6)
    c = torch.einsum("ni,nij->nj", d, camrot[cam_ind])
    u = K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2]
    v = K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]
    seen = (c[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    sx, sy = u - 0.5, v - 0.5
    fx, fy = torch.floor(sx), torch.floor(sy)
    wx, wy = (sx - fx)[:, None], (sy - fy)[:, None]
    x0, x1 = fx.long().clamp(0, W - 1), (fx.long() + 1).clamp(0, W - 1)
    y0, y1 = fy.long().clamp(0, H - 1), (fy.long() + 1).clamp(0, H - 1)

    def tap(y, x):
        return images[cam_ind, y, x].float() / 255.0

    top = (1 - wx) * tap(y0, x0) + wx * tap(y0, x1)
    bot = (1 - wx) * tap(y1, x0) + wx * tap(y1, x1)
    return dirs, torch.where(seen[:, None], (1 - wy) * top + wy * bot, torch.zeros_like(top)), seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--disc", type=float, default=0.3, help="silhouette radius as a share of the image size")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, W = a.views, a.size, a.size
    pts = torch.from_numpy(S.lego_like_points(a.points, seed=0)).to(dev)
    cams = [S.camera(360.0 * f / F, -30.0, 4.0) for f in range(F)]
    campos, camrot = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    focal = S.lego_focal(800) * H / 800.0
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]])
    images = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev,
                           generator=torch.Generator(device=dev).manual_seed(0))
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = ((x + 0.5 - W / 2) ** 2 + (y + 0.5 - H / 2) ** 2 <= (a.disc * W) ** 2)
    alphas = (disc.to(torch.uint8) * 255)[None].expand(F, H, W).contiguous()
    fs = FrameSet(images, (campos, camrot), K, 2.0, 6.0, device=dev)

    res = {"points": a.points, "views": F, "size": H}
    out = SD.seed_points(pts, fs, alphas=alphas, embedding="zeros")
    res["survivors"] = int(out["xyz"].shape[0])
    bits = SD.alpha_bits(alphas, fs)
    kept = out["xyz"]
    t = lambda fn: round(timed(fn, a.warmup, a.repeats), 3)  # noqa: E731
    res["hip_ms"] = {
        "seed_points": t(lambda: SD.seed_points(pts, fs, alphas=alphas, embedding="zeros")),
        "alpha_bits": t(lambda: SD.alpha_bits(alphas, fs)),
        "seed_mask+compact": t(lambda: SD.seed_mask(pts, fs, bits)),
        "seed_view": t(lambda: SD.seed_view(kept, fs)),
    }
    if not a.no_torch:
        Kt = torch.from_numpy(K).float().to(dev)
        pos_t, rot_t = torch.from_numpy(campos).to(dev), torch.from_numpy(camrot).to(dev)
        c2w = torch.eye(4, device=dev).repeat(F, 1, 1)
        c2w[:, :3, :3], c2w[:, :3, 3] = rot_t, pos_t
        w2cs = torch.inverse(c2w)
        al_f = alphas.float() / 255.0
        cx = torch.tensor([W // 2 + 0.5 - W / 2, H // 2 + 0.5 - H / 2, focal], device=dev) / focal
        camdir = torch.einsum("fij,j->fi", rot_t, cx)
        camdir = camdir / (camdir.norm(dim=-1, keepdim=True) + 1e-5)
        hull = torch_alpha_masking(pts, al_f, Kt, w2cs)
        kept_t = pts[hull]
        ind_t = torch_nearest_view(pos_t, camdir, kept_t)
        res["torch_survivors"] = int(kept_t.shape[0])
        res["cam_ind_agree"] = (round(float((ind_t == out["cam_ind"].long()).float().mean()), 5)
                                if kept_t.shape[0] == kept.shape[0] else None)
        res["torch_ms"] = {
            "alpha_masking": t(lambda: torch_alpha_masking(pts, al_f, Kt, w2cs)),
            "nearest_view": t(lambda: torch_nearest_view(pos_t, camdir, kept_t)),
            "lookup": t(lambda: torch_lookup(kept_t, ind_t, images, pos_t, rot_t, Kt)),
        }
        res["torch_ms"]["total"] = round(sum(res["torch_ms"].values()), 3)
        res["speedup"] = round(res["torch_ms"]["total"] / res["hip_ms"]["seed_points"], 2)
    # traffic model: 12 B per point, one 4 B bit-plane word per point and view
    res["mask_model"] = {"point_MB": round(12 * a.points / 1e6, 1), "bit_planes_MB": round(bits.numel() * 4 / 1e6, 1),
                         "probes_M": round(a.points * F / 1e6, 1)}
    assert math.isfinite(res["hip_ms"]["seed_points"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
