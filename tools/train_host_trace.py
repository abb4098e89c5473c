#!/usr/bin/env python3
"""Characterise the training host layer: for each case, the
ordered names of the libpnr entry points one forward + backward calls and the
sha256 of ray_color / features, the point-table gradients and the 16 aggregator
gradients.  Two trees compute the same when their outputs are equal line by line.

    python tools/train_host_trace.py [--root TREE] [--save OUT.npz] > trace.txt
    python tools/train_host_trace.py --diff A.npz B.npz

--root: the tree whose pointnerf_amd is traced (default: this file's); the scenes
and golden inputs are taken from the same tree.  PNR_LIB points both trees at one
libpnr.so.  Only names every version of the package has are used:
render_rays_train, PointAggregator.forward, train.NATIVE_BWD / train.BWD_H2.
--diff: the arrays of two --save files that are not bitwise equal, each with
max |a - b| / max |b|.
"""
import argparse
import gc
import hashlib
import os
import sys

import numpy as np


def diff(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two files hold different arrays"
    n_diff = 0
    for k in a.files:
        if a[k].tobytes() != b[k].tobytes():
            n_diff += 1
            rel = float(np.abs(a[k].astype(np.float64) - b[k]).max()) / max(float(np.abs(b[k]).max()), 1e-30)
            print(f"{k}: max |a - b| / max |b| = {rel:.3e}")
    print(f"{n_diff} of {len(a.files)} arrays differ")


class _Recorder:
    """Stands in for the loaded library: records the name of every entry point
    fetched from it while a case runs, and hands out the real function."""

    def __init__(self, real):
        self._real, self.names, self.on = real, [], False

    def __getattr__(self, name):
        if self.on:
            self.names.append(name)
        return getattr(self._real, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--save")
    ap.add_argument("--diff", nargs=2)
    args = ap.parse_args()
    if args.diff:
        return diff(*args.diff)
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")]
    import torch
    from formula import UPSTREAM_SHAPES, formula_params
    from scenes import scene

    import pointnerf_amd.train as T
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    assert os.path.dirname(os.path.abspath(L.__file__)) == os.path.join(root, "pointnerf_amd")

    cuda = torch.device("cuda:0")
    rec = _Recorder(L.lib())
    L.lib = lambda: rec
    saved = {}

    def report(case, arrays):
        print(f"== {case}")
        print("calls: " + " ".join(rec.names))
        for k, t in arrays.items():
            a = np.ascontiguousarray(t.detach().cpu().numpy())
            saved[f"{case}/{k}"] = a
            print(f"{k}: {hashlib.sha256(a.tobytes()).hexdigest()}")

    def trace(fn):
        # earlier cases' grids are freed (pnr_destroy, from a finaliser) before the case, not at
        # whichever allocation inside it happens to start a collection
        gc.collect()
        torch.cuda.synchronize()
        gc.disable()
        rec.names, rec.on = [], True
        try:
            return fn()
        finally:
            torch.cuda.synchronize()
            rec.on = False
            gc.enable()

    def renderer_case(case, precision, xyz_grad=False, native=True, bwd_h2=True, conf=True, budget=None, C=128):
        T.NATIVE_BWD, T.BWD_H2 = native, bwd_h2
        over = dict(shading_color_channel_num=3) if C == 3 else {}
        sc = scene(20000, H=32, W=32, theta=60.0, default_conf=None, **over)
        if C == 3:
            sc["bg"] = np.array([1.0, 1.0, 1.0], np.float32)
        sc["opt"].xyz_grad = int(xyz_grad)
        params = formula_params(UPSTREAM_SHAPES, salt=0.3) if C == 3 else formula_params(salt=0.3)
        agg = PointAggregator(sc["opt"]).to(cuda)
        agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                           torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]),
                           torch.from_numpy(sc["conf"]) if conf else None)
        m = NeuralPointsRayMarching(sc["opt"], np_, agg.train(), precision="fp32")
        m.train_precision = precision
        m.train_memory_budget = budget
        cp, cr = torch.from_numpy(sc["campos"]).to(cuda), torch.from_numpy(sc["camrot"]).to(cuda)
        rd, bg = torch.from_numpy(sc["raydir"]).to(cuda), torch.from_numpy(sc["bg"]).to(cuda)

        def step():
            color = m.render_rays_train(cp, cr, rd, 2.0, 6.0, bg)[0]
            G = torch.randn(color.shape, generator=torch.Generator().manual_seed(5)).to(cuda)
            (color * G).sum().backward()
            return color

        color = trace(step)
        out = {"ray_color": color}
        for k in ("points_embeding", "points_color", "points_dir", "points_conf", "xyz"):
            p = getattr(np_, k)
            if p is not None and p.grad is not None:
                out["d " + k] = p.grad
        out.update({"d " + k: p.grad for k, p in agg.named_parameters() if p.grad is not None})
        report(f"{case} count_reads={m.train_count_reads} h2_fallbacks={m.h2_fallbacks}", out)
        T.NATIVE_BWD, T.BWD_H2 = True, True

    def seam_case(case, per_pair):
        g = np.load(os.path.join(root, "tests", "golden", "aggregator_rw2c.npz"), allow_pickle=False)
        agg = PointAggregator(lego_opt()).to(cuda)
        agg.load_state_dict({k: torch.from_numpy(v) for k, v in formula_params(salt=0.3).items()})
        agg.train()
        names = ("sampled_color", "sampled_Rw2c", "sampled_dir", "sampled_conf", "sampled_embedding",
                 "sampled_xyz_pers", "sampled_xyz", "sample_pnt_mask", "sample_loc", "sample_loc_w", "sample_ray_dirs")
        t = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(cuda) for k in names}
        if not per_pair:
            t["sampled_Rw2c"] = t["sampled_Rw2c"].reshape(-1, 3, 3)[0].contiguous()
        leaves = ("sampled_color", "sampled_dir", "sampled_conf", "sampled_embedding")
        for k in leaves:
            t[k].requires_grad_(True)

        def step():
            f = agg(*(t[k] for k in names), [0.004] * 3, 0)[0]
            G = torch.randn(f.shape, generator=torch.Generator().manual_seed(5)).to(cuda)
            (f * G).sum().backward()
            return f

        f = trace(step)
        out = {"features": f}
        out.update({"d " + k: t[k].grad for k in leaves})
        out.update({"d " + k: p.grad for k, p in agg.named_parameters() if p.grad is not None})
        report(case, out)

    for prec in ("fp32", "fp32x3", "fp32h2"):
        for xg in (False, True):
            renderer_case(f"renderer {prec} xyz_grad={int(xg)}", prec, xyz_grad=xg)
    renderer_case("renderer fp32h2 NATIVE_BWD=False", "fp32h2", native=False)
    renderer_case("renderer fp32h2 BWD_H2=False", "fp32h2", bwd_h2=False)
    renderer_case("renderer fp32h2 points_conf=None", "fp32h2", conf=False)
    renderer_case("renderer fp32h2 train_memory_budget=1MiB", "fp32h2", budget=1 << 20)
    renderer_case("renderer fp32h2 rgb_head", "fp32h2", C=3)
    seam_case("seam per-pair Rw2c", True)
    seam_case("seam uniform Rw2c", False)
    if args.save:
        np.savez(args.save, **saved)


if __name__ == "__main__":
    main()
