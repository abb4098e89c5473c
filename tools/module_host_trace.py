#!/usr/bin/env python3
"""Characterise the module's host layer: for each case, the
ordered names of the libpnr entry points the call fetches and the sha256 of every
output.  Two trees compute the same when their outputs are equal line by line.

    python tools/module_host_trace.py [--root TREE] [--save OUT.npz] > trace.txt
    python tools/module_host_trace.py --diff A.npz B.npz

--root: the tree whose pointnerf_amd is traced (default: this file's); the scenes
are taken from the same tree.  PNR_LIB points both trees at one libpnr.so.  Only
names every version of the package has are used: the module's forward,
render_rays, finish, render_views, render_pixels, probe_rays, RenderGraph.
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
    from formula import formula_params
    from scenes import scene

    import pquery_frame_ref as FR
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching, RenderGraph
    from test_gpu_pquery_render import inputs as pinputs
    assert os.path.dirname(os.path.abspath(L.__file__)) == os.path.join(root, "pointnerf_amd")

    cuda = torch.device("cuda:0")
    rec = _Recorder(L.lib())
    L.lib = lambda: rec
    saved = {}

    def report(case, arrays):
        print(f"== {case}")
        print("calls: " + " ".join(rec.names))
        for k, t in arrays.items():
            if not torch.is_tensor(t):
                print(f"{k}: {t!r}")
                continue
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

    def model(sc, precision="fp32h2", train=False, **kw):
        agg = PointAggregator(sc["opt"]).to(cuda)
        agg.load_state_dict({k: torch.from_numpy(v) for k, v in formula_params(salt=0.3).items()})
        np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                           torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]))
        return NeuralPointsRayMarching(sc["opt"], np_, agg.train() if train else agg.eval(), precision=precision, **kw)

    def world(**opt_over):
        sc = scene(20000, H=32, W=32, theta=60.0, default_conf=None, **opt_over)
        t = {k: torch.from_numpy(sc[k]).to(cuda) for k in ("campos", "camrot", "raydir", "bg")}
        return sc, (t["campos"], t["camrot"], t["raydir"], 2.0, 6.0, t["bg"])

    def named(out, prefix=""):
        return {f"{prefix}{k}": t for k, t in zip(("ray_color", "opacity", "is_bg", "ray_mask"), out)}

    items = {"": [], " aux": ["conf_coefficient"]}

    # forward on each of the four routes, with and without the aux outputs
    for tag, zo in items.items():
        for train in (False, True):
            sc, a = world(zero_one_loss_items=zo)
            m = model(sc, train=train).train(train)
            kw = dict(campos=a[0][None], raydir=a[2][None], bg_color=a[5], camrotc2w=a[1][None],
                      near=torch.tensor([[2.0]], device=cuda), far=torch.tensor([[6.0]], device=cuda))
            with torch.set_grad_enabled(train):
                out = trace(lambda: m(**kw))
            report(f"forward world {'train' if train else 'eval'}{tag}", out)
        for fused in (False, True):
            sc = FR.scene("C")
            sc["opt"].zero_one_loss_items = zo
            m = model(sc, "fp32", fused_perspective=fused)
            kw = pinputs(sc, cuda)
            with torch.no_grad():
                out = trace(lambda: m(**kw))
            report(f"forward perspective fused_perspective={fused}{tag}", out)

    # render_rays in every precision, the batch split in three chunks
    sc, a = world()
    for prec in ("fp32", "fp32x3", "fp32h2", "bf16"):
        m = model(sc, prec, chunk_rays=-(-a[2].shape[0] // 3))
        ev = []
        out = trace(lambda: m.render_rays(*a, events=ev))
        report(f"render_rays {prec} 3 chunks events={'/'.join(e[0] for e in ev)} counts={m.last_counts}", named(out))

    # two sync=False calls, finish(upto=1), finish()
    m = model(sc)
    m.render_rays(*a)

    def queued():
        o1, o2 = m.render_rays(*a, sync=False), m.render_rays(*a, sync=False)
        c1 = m.finish(upto=1)
        return o1, o2, c1, m.finish()

    o1, o2, c1, c2 = trace(queued)
    report(f"queued x2 finish(upto=1)={c1} finish()={c2}", {**named(o1, "first "), **named(o2, "second ")})

    # a call whose feature buffer overflows its estimate: re-rendered by finish()
    m._sv_per_ray = 0.01

    def overflow():
        o = m.render_rays(*a, sync=False)
        return o, m.finish()

    o, c = trace(overflow)
    report(f"overflow rerender counts={c} overflow_rerenders={m.overflow_rerenders} h2_fallbacks={m.h2_fallbacks}",
           named(o))

    # render_views: two views as one batch
    sc2, a2 = world()
    m = model(sc)
    half = a[2].shape[0] // 2
    views = [(a[0], a[1], a[2][:half]), (a2[0], a2[1], a[2][half:])]
    outs = trace(lambda: m.render_views(views, 2.0, 6.0, a[5]))
    report("render_views x2", {**named(outs[0], "view0 "), **named(outs[1], "view1 ")})

    # render_pixels in its three precisions
    scp = FR.scene("C")
    inp = pinputs(scp, cuda)
    pa = (inp["campos"][0], inp["camrotc2w"][0], inp["pixel_idx"][0], scp["H"], scp["W"], inp["intrinsic"][0], 2.0, 6.0,
          inp["bg_color"])
    for prec in ("fp32", "fp32x3", "fp32h2"):
        m = model(scp, prec, chunk_rays=500)
        ev = []
        out = trace(lambda: m.render_pixels(*pa, events=ev))
        report(f"render_pixels {prec} events={'/'.join(e[0] for e in ev)} counts={m.last_counts}", named(out))

    # probe_rays
    m = model(sc, chunk_rays=400)
    out = trace(lambda: m.probe_rays(*a))
    report("probe_rays", out)

    # RenderGraph: build, replay, check
    m = model(sc)
    m.render_rays(*a)

    def graph():
        g = RenderGraph(m, *a)
        out = g.replay()
        return out, g.check(), g.last_counts

    out, ok, counts = trace(graph)
    report(f"RenderGraph check={ok} counts={counts}", named(out))
    if args.save:
        np.savez(args.save, **saved)


if __name__ == "__main__":
    main()
