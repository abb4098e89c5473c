"""Dev tool: time the perspective-frustum query on one DTU-shaped
frame -- 640 x 512, options.dtu_opt (vscale 2 2 1, SR 40, K 8, P 20,
z_depth_dim 400, near 2, far 4.725) -- over a lego-like cloud scaled so that
its depths fall inside near..far, next to the world-grid query (grid build and
query apart) of the same cloud and the same number of rays.  HIP events,
warm-up, median of --repeats.  Prints one JSON line with the call times, the
query's stats, the bytes its kernels must move (computed from the shapes) and
the shader clock under load.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats` with --repeats 5.

--frame times the whole evaluation frame on the same inputs instead (DESIGN.md
29): render_pixels (the fused perspective frame) for fp32 and fp32h2, with its
stage events, next to the module's seam forward in eval mode -- the same
timing rule -- and the peak device memory of each
(torch.cuda.max_memory_allocated).  --out writes the JSON to a file as well."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pointnerf_amd import _lib as L  # noqa: E402
from pointnerf_amd import synthetic as S  # noqa: E402
from pointnerf_amd.options import dtu_opt, lego_opt  # noqa: E402
from pointnerf_amd.querier import lighting_fast_querier as WorldQuerier  # noqa: E402
from pointnerf_amd.querier_p import frustum_geometry, lighting_fast_querier, pquery_params  # noqa: E402


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


def frame_bench(a, dev, opt, xyz, cp, cr, K, pix):
    """render_pixels (fp32, fp32h2) and the seam forward on one frame -> dict."""
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    W, H, N = a.width, a.height, a.points
    torch.manual_seed(0)
    emb, color, dirs, conf = S.point_features(N, seed=0)
    agg = PointAggregator(opt).to(dev).eval()
    np_ = NeuralPoints(opt, dev, xyz, emb, color, dirs, conf)
    bg = torch.rand(agg.C, generator=torch.Generator().manual_seed(1)).to(dev)
    args = (cp, cr, pix, H, W, K, opt.near_plane, opt.far_plane, bg)
    res = {"points": N, "frame": [W, H], "rays": W * H, "hip_ms": {}, "stage_ms": {}, "peak_MB": {}, "counts": {},
           "lib": os.path.basename(L.LIB_PATH), "warmup": a.warmup, "repeats": a.repeats}
    outs = {}
    for prec in ("fp32", "fp32h2"):
        m = NeuralPointsRayMarching(opt, np_, agg, precision=prec)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        with torch.no_grad():
            res["hip_ms"][f"render_pixels {prec}"] = timed(lambda: m.render_pixels(*args), a.warmup, a.repeats)
            peak = torch.cuda.max_memory_allocated(dev) - base
            res["peak_MB"][f"render_pixels {prec}"] = round(peak / 1e6, 1)
            stages = {}
            for _ in range(a.repeats):
                ev = []
                outs[prec] = m.render_pixels(*args, events=ev)
                torch.cuda.synchronize()
                for name, e0, e1 in ev:
                    stages.setdefault(name, []).append(e0.elapsed_time(e1))
        res["stage_ms"][prec] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in stages.items()}
        res["counts"][prec] = dict(m.last_counts, h2_fallbacks=m.h2_fallbacks)
        del m
    a32, ah2 = outs["fp32"], outs["fp32h2"]
    res["fp32h2_vs_fp32_max_abs"] = {"ray_color": float((a32[0] - ah2[0]).abs().max()),
                                     "opacity": float((a32[1] - ah2[1]).abs().max())}
    # the seam forward of the same model (NeuralPoints.forward's gathers, PointAggregator.forward, torch march)
    m = NeuralPointsRayMarching(opt, np_, agg, precision="fp32").eval()
    raydir = torch.from_numpy(S.pixel_rays(H, W, float(K[0, 0]), cr.cpu().numpy())).to(dev)
    t = lambda v: torch.tensor([[v]], device=dev)   # noqa: E731
    inp = dict(campos=cp[None], raydir=raydir[None], bg_color=bg, camrotc2w=cr[None],
               pixel_idx=pix[None].long(),
               near=t(opt.near_plane), far=t(opt.far_plane), h=torch.tensor([H], device=dev),
               w=torch.tensor([W], device=dev), intrinsic=torch.from_numpy(K).to(dev)[None])
    seam_out = {}

    def seam():
        seam_out["o"] = None   # the previous frame's tensors are freed before the next one's are allocated
        seam_out["o"] = m(**inp)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    with torch.no_grad():
        res["hip_ms"]["seam forward (eval)"] = timed(seam, a.warmup, a.repeats)
    res["peak_MB"]["seam forward (eval)"] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)
    o = seam_out["o"]
    res["fused_vs_seam_max_abs"] = {"ray_color": float((a32[0] - o["coarse_raycolor"][0]).abs().max()),
                                    "opacity": float((a32[1] - o["coarse_point_opacity"][0]).abs().max()),
                                    "ray_mask_equal": bool(torch.equal(a32[3], o["ray_mask"][0]))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--scale", type=float, default=0.6, help="cloud scale: depths 3.3 .. 4.7 from the radius-4 camera")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frame", action="store_true", help="time the whole frame: render_pixels and the seam forward")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, N = a.width, a.height, a.points
    opt = dtu_opt()
    xyz = torch.from_numpy(S.lego_like_points(N, seed=0) * np.float32(a.scale)).to(dev)
    campos, camrot = S.camera(30.0, -30.0, 4.0)
    focal = S.lego_focal(800) * W / 800.0 / a.scale          # the scaled cloud fills the frame as lego does
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], np.float32)
    cp, cr = torch.from_numpy(campos).to(dev), torch.from_numpy(camrot).to(dev)
    xc = (xyz - cp) @ cr
    pers = torch.stack([xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2], xc[:, 2]], -1).contiguous()
    px, py = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    pix = torch.from_numpy(np.stack([px, py], -1).reshape(-1, 2)).to(dev)
    R, SR, Kn = W * H, opt.SR, opt.K
    if a.frame:
        return emit(frame_bench(a, dev, opt, xyz, cp, cr, K, pix), a.out)

    q = lighting_fast_querier(dev, opt)
    seam = lambda: q.query_points(pix[None], pers[None], xyz[None], None, H, W, K, opt.near_plane, opt.far_plane,  # noqa: E731
                                  None, cp[None], cr[None])
    out = seam()
    stats = q.stats()
    Rv = int(out[0].shape[1])
    res = {"points": N, "frame": [W, H], "rays": R, "rays_hit": Rv, "stats": stats,
           "samples_filled": int((out[0][..., 0] >= 0).sum()), "lib": os.path.basename(L.LIB_PATH)}

    # the ABI call on its own, buffers preallocated
    geo = frustum_geometry(opt, H, W, K, opt.near_plane, opt.far_plane)
    qp = pquery_params(opt, geo)
    i32 = dict(dtype=torch.int32, device=dev)
    rows_pidx, rows_loc = torch.empty((R, SR, Kn), **i32), torch.empty((R, SR, 3), device=dev)
    rows_z, mask = torch.empty((R, SR), **i32), torch.empty(R, dtype=torch.int8, device=dev)
    counts, st_dev = torch.zeros(4, **i32), torch.zeros(8, **i32)
    dims = (L.c_int32 * 3)(*[int(v) for v in geo.dims])
    scr = L.scratch("pnr_pquery_scratch_bytes", N, R, SR, dims, device=dev)
    st = L.stream_ptr(dev)

    def call():
        L.check(L.lib().pnr_pquery(L.ctypes.byref(qp), L.ptr(pers), N, L.ptr(pix), R, L.ptr(rows_pidx), L.ptr(rows_loc),
                                   L.ptr(rows_z), L.ptr(mask), L.ptr(counts), L.ptr(st_dev), L.ptr(scr), scr.numel(), st),
                "pnr_pquery")

    clock = torch.zeros(1, device=dev)
    side = torch.cuda.Stream(dev)
    res["hip_ms"] = {"query_points (seam, with pers2w)": timed(seam, a.warmup, a.repeats),
                     "pnr_pquery": timed(call, a.warmup, a.repeats)}
    for _ in range(3):
        call()
    with torch.cuda.stream(side):   # the shader clock one wave sees while the queued queries run
        L.check(L.lib().pnr_clock_probe(L.ptr(clock), 4000, L.stream_ptr(dev)), "pnr_clock_probe")
    torch.cuda.synchronize()
    res["sclk_mhz_under_load"] = round(float(clock[0]), 1)

    # bytes the algorithm needs (reads + writes), from the shapes
    cols, wz = int(geo.dims[0] * geo.dims[1]), (int(geo.dims[2]) + 31) // 32
    listed = stats["n_points_in_grid"]
    res["scratch_MB"] = round(scr.numel() / 1e6, 1)
    res["model_MB"] = {
        "bin": round((N * 12 + N * 8) / 1e6, 1),
        "scatter": round((N * 8 + listed * 8) / 1e6, 1),
        "dilate": round(cols * wz * 4 * (9 * 3 + 1) / 1e6, 1),
        "column": round((listed * (8 + 8 + 12 + 20)) / 1e6, 1),
        "select": round((R * (8 + 5) + cols * wz * 4) / 1e6, 1),
        "knn_writes": round(Rv * SR * (Kn * 4 + 12 + 4) / 1e6, 1),
    }

    # the world-grid query of the same cloud and as many rays, for scale
    wopt = lego_opt(ranges=[v * a.scale for v in lego_opt().ranges], SR=SR, P=opt.P)
    wq = WorldQuerier(dev, wopt)
    raydir = torch.from_numpy(S.pixel_rays(H, W, float(focal), camrot)).to(dev)
    bufs = None

    def world_query():
        nonlocal bufs
        bufs = wq.run(xyz, raydir, cp, cr, opt.near_plane, opt.far_plane, bufs=bufs)[0]

    world_query()
    res["world"] = {"counts": bufs.read_counts(), "grid": wq.grid.stats()}
    res["hip_ms"]["world query (grid cached)"] = timed(world_query, a.warmup, a.repeats)
    res["hip_ms"]["world grid build"] = timed(lambda: wq.grid.build(wopt, xyz, force=True), a.warmup, a.repeats)
    emit(res, a.out)


def emit(res, out):
    line = json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
