#!/usr/bin/env python3
"""Characterise the grid host layer: for each case, the
ordered names of the libpnr entry points one build + query calls and the sha256
of the exported tables, the hp entries, stats() and the query's outputs.  The
build is deterministic and uses no float atomics, so two trees compute the same
only when their outputs are equal line by line.

    python tools/grid_host_trace.py [--root TREE] [--save OUT.npz] > trace.txt
    python tools/grid_host_trace.py --diff A.npz B.npz

--root: the tree whose pointnerf_amd (and libpnr.so) is traced (default: this
file's); the scenes are taken from the same tree.  Only names every version of
the package has are used: lighting_fast_querier, GridHandle.build / export /
stats / query, QueryBuffers, make_rays, camera_tables.
--diff: the arrays of two --save files that are not bitwise equal.
"""
import argparse
import gc
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np


def diff(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two files hold different arrays"
    bad = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    for k in bad:
        print(f"{k}: differs")
    print(f"{len(bad)} of {len(a.files)} arrays differ")
    return 1 if bad else 0


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
    from scenes import flag_scene, scene

    from pointnerf_amd import _lib as L
    from pointnerf_amd.querier import QueryBuffers, camera_tables, lighting_fast_querier, make_rays
    assert os.path.dirname(os.path.abspath(L.__file__)) == os.path.join(root, "pointnerf_amd")

    cuda = torch.device("cuda:0")
    rec = _Recorder(L.lib())
    L.lib = lambda: rec
    saved = {}

    def case(name, sc, xyz=None, R=None, near=2.0, far=6.0, **opt_over):
        opt = SimpleNamespace(**{**vars(sc["opt"]), **opt_over})
        xyz = torch.from_numpy(sc["xyz"] if xyz is None else xyz).to(cuda)
        rd = torch.from_numpy(sc["raydir"]).to(cuda)
        cp, cr = torch.from_numpy(sc["campos"]).to(cuda), torch.from_numpy(sc["camrot"]).to(cuda)
        gc.collect()   # earlier cases' handles go now (pnr_destroy from release_deferred), not inside the case
        q = lighting_fast_querier(cuda, opt)
        torch.cuda.synchronize()
        gc.disable()
        torch.manual_seed(3)   # the jittered depths of is_train
        rec.names, rec.on = [], True
        try:
            if R == 0:   # pnr_rays.R = 0 with live pointers (an empty slice of raydir has none)
                hp = q.grid.build(opt, xyz)
                rays = make_rays(*camera_tables(cp, cr), rd, q.tvals(near, far, 0, cuda)[0], False)
                rays.R = 0
                bufs = QueryBuffers(0, opt.SR, opt.K, cuda)
                q.grid.query(opt, hp, rays, bufs)
            else:
                bufs, hp, _, _ = q.run(xyz, rd, cp, cr, near, far)
            tables = q.grid.export()
            st = q.grid.stats()
            out = {"hp " + k: np.asarray(hp[k]) for k in ("shift", "dims", "ranges", "vsize_s", "radius_limit2")}
            torch.cuda.synchronize()
        finally:
            rec.on = False
            gc.enable()
        out.update({"table " + k: v for k, v in tables.items()})
        out["stats"] = np.array([st[k] for k in ("n_points_in_grid", "n_voxels", "n_voxels_kept", "n_points_dropped",
                                                 "max_points_per_voxel", "table_cells")] + list(st["dims"]), np.int64)
        c = bufs.read_counts()
        S = c["S_filled"]
        out["counts"] = bufs.counts.cpu().numpy()
        out["pidx"] = bufs.pidx[: S * opt.K]
        out["sample_w"], out["sample_p"] = bufs.sample_w[: S * 3], bufs.sample_p[: S * 3]
        out["valid_list"] = bufs.valid_list[: c["S_valid"]]
        print(f"== {name} hp={type(hp).__name__}")
        print("calls: " + " ".join(rec.names))
        for k, t in out.items():
            a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
            saved[f"{name}/{k}"] = a
            print(f"{k}: {hashlib.sha256(a.tobytes()).hexdigest()}")
        q.clean_up()

    ray = dict(H=24, W=24, theta=70.0)
    for n, max_o, P in [(20000, 1500, 1), (3, 8, 2), (70000, 400000, 9)]:
        for drop in (0, 1):
            sc = scene(max(n, 20000), max_o=max_o, P=P, slot0_drop=drop, **ray)
            case(f"sizes n={n} max_o={max_o} P={P} slot0_drop={drop}", sc, xyz=sc["xyz"][:n].copy())
    sc = scene(20000, **ray)
    clouds = {"inside": sc["xyz"], "crossing": sc["xyz"].copy(),
              "shifted": (sc["xyz"] * 0.4 + np.array([0.35, 0.6, 0.6], np.float32)).astype(np.float32)}
    clouds["crossing"][::7] *= 1.6
    for cname, xyz in clouds.items():
        for host in (False, True):
            case(f"geometry {cname} grid_host_bbox={host}", sc, xyz=xyz, grid_host_bbox=host)
    case("grow n > max_o", scene(20000, max_o=1500, **ray), max_o_policy="grow")
    tr = flag_scene("truck", n_points=20000, H=24)
    case("truck kernel 5", tr, near=tr["near"], far=tr["far"])
    for K in (4, 8, 16):
        case(f"K={K}", scene(20000, K=K, **ray))
    case("jittered tvals", scene(20000, is_train=1, **ray))
    case("R=0", sc, R=0)
    if args.save:
        np.savez(args.save, **saved)


if __name__ == "__main__":
    sys.exit(main())
