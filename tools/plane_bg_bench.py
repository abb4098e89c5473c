"""Dev tool: time the plane background on a DTU-sized synthetic
frame: 512 x 640 rays against F source views of 512 x 640 (uint8) and a
300 k-point cloud standing on a tilted table plane whose images are made by
projecting the plane.  pnr_plane_fg_masks and pnr_plane_bg are timed with HIP
events around 20 launches, next to the same result computed the reference's
way with torch ops on the same GPU: per view a projection, ceil and index_put
for the masks (mvs_utils.homo_warp_fg_mask), and per view one grid_sample of
the in-bounds, uncovered points, a masked scatter, then the fit mask and the
max over views (set_bg, models/mvs_points_volumetric_model.py:279-317; its
grid_sample runs on the CPU there, on the GPU here).  The two formulations
alternate, sample by sample.  Prints one JSON line; --out also writes it."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F_

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pointnerf_amd import PlaneBackground  # noqa: E402
from pointnerf_amd.rays import FrameSet, camera_rays  # noqa: E402

PLANE_PNT = np.array([0.1, -0.05, -0.2])
PLANE_NORMAL = np.array([0.15, -0.1, -1.0])
LEVELS = np.array([153, 128, 102])
LAUNCHES = 20


def look_at(pos, target):
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd], 1)


def ring(Fv, radius=3.0):
    pos, rot = [], []
    for f in range(Fv):
        az, el = 2 * np.pi * f / Fv + 0.3, 0.75 + 0.2 * math.sin(3 * (2 * np.pi * f / Fv + 0.3))
        c = PLANE_PNT + radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        t = PLANE_PNT + 0.3 * np.array([math.cos(2.4 * f + 1.0), math.sin(2.4 * f + 1.0), 0.0])
        pos.append(c)
        rot.append(look_at(c, t))
    return np.array(pos), np.array(rot)


def plane_images(pos, rot, K, H, W, dev, disc=1.0):
    """[F,H,W,3] uint8 on the device: the plane colour (a few levels off per
    view; view 2 off by 13) within ``disc`` of the plane point, a smooth pattern
    elsewhere."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                          torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    pattern = torch.stack([0.15 + 0.1 * torch.sin(x / 50), 0.5 + 0.3 * torch.cos(y / 40),
                           0.8 + 0.1 * torch.sin((x + y) / 60)], -1)
    n, p0 = torch.tensor(PLANE_NORMAL, device=dev), torch.tensor(PLANE_PNT, device=dev)
    out = torch.empty((len(pos), H, W, 3), dtype=torch.uint8, device=dev)
    offsets = np.array([0, 2, -3, 5])
    for f in range(len(pos)):
        dc = torch.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], torch.ones_like(x)], -1)
        d = dc @ torch.tensor(rot[f], device=dev).T
        c = torch.tensor(pos[f], device=dev)
        t = (n @ (p0 - c)) / (d @ n)
        on = (t > 0) & ((c + d * t[..., None] - p0).norm(dim=-1) < disc)
        lv = LEVELS + (13 if f == 2 else offsets[(f + np.arange(3)) % 4] * (f > 0))
        out[f] = torch.where(on[..., None], torch.tensor(lv, device=dev, dtype=torch.float64),
                             torch.round(pattern * 255)).to(torch.uint8)
    return out


def event_ms(fn, launches):
    """ms per call: HIP events around ``launches`` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "samples": len(v)}


# ------------------------------------------------- the reference's formulation
def torch_project(p, w2c, K):
    cam = p @ w2c[:3, :3].T + w2c[:3, 3]
    return ((cam / cam[:, 2:3]) @ K.T)[:, :2]


def torch_fg_masks(xyz, w2cs, K, H, W):
    out = []
    hi = torch.tensor([W - 1.0, H - 1.0], device=xyz.device)
    for w2c in w2cs:
        g = torch_project(xyz, w2c, K)
        m = ((g >= 0) & (g <= hi)).all(-1)
        ids = torch.ceil(g[m]).long()
        mask = torch.zeros((H, W), dtype=torch.int8, device=xyz.device)
        mask[ids[:, 1], ids[:, 0]] = 1
        out.append(mask)
    return torch.stack(out)


def torch_plane_bg(campos, raydir, p0, n, color, imgs, w2cs, K, fg, H, W, count=None):
    dot = (n * raydir).sum(-1)
    board = dot >= 1e-3
    fac = -(n * (campos - p0)).sum(-1) / dot[board]
    p = torch.zeros_like(raydir)
    p[board] = campos + raydir[board] * fac[:, None]
    hi = torch.tensor([W - 1.0, H - 1.0], device=p.device)
    feats = []
    for f, w2c in enumerate(w2cs):
        g = torch_project(p, w2c, K)
        m = ((g >= 0) & (g <= hi)).all(-1)
        ids = torch.ceil(g[m]).long()
        m[m.clone()] = fg[f][ids[:, 1], ids[:, 0]] < 1
        if count is not None:
            count.append(m.sum())
        grid = g[m]
        grid = torch.stack([grid[:, 0] / ((W - 1.0) / 2.0) - 1.0, grid[:, 1] / ((H - 1.0) / 2.0) - 1.0], -1)
        s = F_.grid_sample(imgs[f:f + 1], grid[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)
        full = torch.zeros_like(raydir)
        full[m] = s[0, :, 0].T
        feats.append(full)
    feats = torch.stack(feats, -2)
    fit = ((feats >= color - 0.03) & (feats <= color + 0.03)).all(-1)
    feats = feats * fit[..., None]
    return feats.max(-2)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[16, 49])
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    res = {"rays": H * W, "points": a.points, "image": [H, W], "launches_per_sample": LAUNCHES, "cases": []}
    for Fv in a.views:
        pos, rot = ring(Fv)
        focal = 1.6 * W
        K = np.array([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1.0]])
        images = plane_images(pos, rot, K, H, W, dev)
        fs = FrameSet(images, (pos, rot), K, 2.0, 6.0, device=dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        up = -PLANE_NORMAL / np.linalg.norm(PLANE_NORMAL)
        side = torch.randn((a.points, 3), generator=gen, device=dev, dtype=torch.float64) * 0.18
        upt = torch.tensor(up, device=dev)
        side = side - (side @ upt)[:, None] * upt
        xyz = (torch.tensor(PLANE_PNT, device=dev) + side
               + upt * torch.rand((a.points, 1), generator=gen, device=dev, dtype=torch.float64) * 0.5).float()
        # the render camera: between two source views, looking at the table
        rc = PLANE_PNT + 2.6 * np.array([math.cos(0.8) * math.cos(1.0), math.cos(0.8) * math.sin(1.0), math.sin(0.8)])
        rrot = look_at(rc, PLANE_PNT)
        rK = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1.0]])
        campos = torch.tensor(rc, device=dev).float()[None]
        raydir = camera_rays(rK, torch.tensor(rrot, device=dev).float(), H, W, device=dev)
        color = (LEVELS.astype(np.float32) / np.float32(255))
        bg = PlaneBackground(fs, PLANE_PNT, PLANE_NORMAL, color, points_xyz=xyz)
        got = bg.rays(campos, raydir)[0]

        c2w = torch.eye(4, device=dev, dtype=torch.float64).repeat(Fv, 1, 1)
        c2w[:, :3, :3], c2w[:, :3, 3] = torch.tensor(rot, device=dev), torch.tensor(pos, device=dev)
        w2cs = torch.inverse(c2w).float()
        Kt = torch.tensor(K, device=dev).float()
        imgs = (images.float() / 255.0).permute(0, 3, 1, 2).contiguous()      # [F,3,H,W] float, made once, untimed
        p0, n, col = (torch.tensor(v, device=dev).float() for v in (PLANE_PNT, PLANE_NORMAL, color))
        fg_t = torch_fg_masks(xyz, w2cs, Kt, H, W)
        pairs = []
        ref = torch_plane_bg(campos, raydir, p0, n, col, imgs, w2cs, Kt, fg_t, H, W, pairs)
        pairs = int(torch.stack(pairs).sum())
        agree_fg = float((fg_t.bool() == bg.fg_masks.bool()).float().mean())
        close = float(((got - ref).abs().max(-1)[0] <= 1e-4).float().mean())

        calls = {
            "pnr_plane_fg_masks": (lambda: bg.refresh_fg(xyz), LAUNCHES),
            "pnr_plane_bg": (lambda: bg.rays(campos, raydir), LAUNCHES),
            "torch_fg_masks": (lambda: torch_fg_masks(xyz, w2cs, Kt, H, W), 2),
            "torch_plane_bg": (lambda: torch_plane_bg(campos, raydir, p0, n, col, imgs, w2cs, Kt, fg_t, H, W), 2),
        }
        for fn, _ in calls.values():      # warm-up: every shape of the timed window
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(a.samples):        # alternate the formulations, sample by sample
            for k, (fn, launches) in calls.items():
                times[k].append(event_ms(fn, launches))
        case = {"views": Fv, **{k: stats(v) for k, v in times.items()}}
        R = H * W
        model_bytes = R * 24 + pairs * (4 * 3 + 1)          # rays in, bg out; per ray and view in play 4 uint8 taps + 1 fg byte
        t_bg = case["pnr_plane_bg"]["median_ms"] * 1e-3
        case.update(
            rays_with_background=int((got != 0).any(-1).sum()), ray_view_pairs_sampled=pairs,
            fg_pixels_set=int(bg.fg_masks.sum()), fg_masks_agree=round(agree_fg, 6), bg_within_1e4_of_torch=round(close, 6),
            model_MB=round(model_bytes / 1e6, 2), achieved_GBps=round(model_bytes / t_bg / 1e9, 1),
            speedup_plane_bg=round(case["torch_plane_bg"]["median_ms"] / case["pnr_plane_bg"]["median_ms"], 1),
            speedup_fg_masks=round(case["torch_fg_masks"]["median_ms"] / case["pnr_plane_fg_masks"]["median_ms"], 1))
        assert math.isfinite(t_bg) and t_bg > 0
        res["cases"].append(case)
        del images, imgs, fs, bg
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
