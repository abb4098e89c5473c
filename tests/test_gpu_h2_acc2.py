"""pnr_aggregate_fwd_h2 with two accumulator sets per layer (main += Wh.Xh,
corr += Wl.Xh + Wh.Xl, y = 2^s (main + 2^-11 corr); aggregate_x3.hip `layer`
ACC2) on seeded random clouds with hand-built samples: some samples have fewer
than 8 neighbours and one has none.

Bound (the one test_gpu_x3.py states), against the oracle evaluated in float64,
with the float32 oracle's own error as the yardstick:
  max |h2 - ref64| <= 2 max |ref32 - ref64| + 1e-7 max|ref64|
  rms              <= 1.5 rms(ref32 - ref64) + 1e-8 max|ref64|

Sample counts: 5 (one partial tile), 2061 (258 tiles > 256 workgroups, not a
multiple of 8: dynamic hand-out and tail), 4229 (529 tiles >= 2*256 + 16: the
XCD-aware schedule; 529 > 2*256, so at least one workgroup runs three tiles and
its double-buffered extras alternate 0, 1, 0)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from formula import formula_params
from oracle import oracle as O

pytestmark = pytest.mark.gpu
K = 8
N_POINTS = 3001   # P1 tiles: not a multiple of 64
EMPTY = 3         # the sample without a neighbour


@contextlib.contextmanager
def _oracle_f64():
    old = O.F32
    O.F32 = np.float64
    try:
        yield
    finally:
        O.F32 = old


def _weights(kind):
    p = dict(formula_params(salt=0.3))
    f = np.float32
    if kind == "scales":
        # per-layer shifts differ: block1.2 near the top of the pre-scaled range
        # (as test_h2_large_weights_prescaled), block3.0 far below, block3.2 between
        p["block1.2.weight"] = p["block1.2.weight"] * f(64.0)
        p["block3.0.weight"] = p["block3.0.weight"] / f(64.0)
        p["block3.0.bias"] = p["block3.0.bias"] / f(64.0)
        p["block3.2.weight"] = p["block3.2.weight"] * f(4.0)
        p["alpha_branch.0.weight"] = p["alpha_branch.0.weight"] / f(4.0)
        p["color_branch.0.weight"] = p["color_branch.0.weight"] / f(4.0)
    elif kind == "cancel":
        # block1.0 rows 2j and 2j + 1 equal -> equal activations; block1.2 columns
        # 2j, 2j + 1 = w, -w (1 + 2^-13): the f16 high halves cancel, the output
        # is carried by the low halves (corr)
        for k in ("block1.0.weight", "block1.0.bias"):
            a = p[k].copy()
            a[1::2] = a[0::2]
            p[k] = a
        w = p["block1.2.weight"].copy()
        w[:, 1::2] = -(w[:, 0::2] * f(1.0 + 2.0 ** -13))
        p["block1.2.weight"] = w
    return p


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """Inputs and both oracle results of one case (computed once, read-only)."""
    from pointnerf_amd import synthetic as S
    from pointnerf_amd.options import lego_opt
    rng = np.random.default_rng(1000 + n)
    xyz = rng.uniform(-0.1, 0.1, (N_POINTS, 3)).astype(np.float32)
    emb, color, dirs, conf = (t.numpy() for t in S.point_features(N_POINTS, seed=5, default_conf=None))
    if kind == "extras":   # block3.0 inputs 256..262 two orders of magnitude above the features
        color, dirs = color * np.float32(100.0), dirs * np.float32(100.0)
    campos, camrot = S.camera(30.0, -30.0, 4.0)
    pidx = rng.integers(0, N_POINTS, (n, K)).astype(np.int32)
    cnt = rng.integers(1, K + 1, n)
    cnt[::5] = K
    pidx[np.arange(K)[None, :] >= cnt[:, None]] = -1
    if n > EMPTY:
        pidx[EMPTY] = -1
    loc_w = (xyz[rng.integers(0, N_POINTS, n)] + rng.uniform(-0.01, 0.01, (n, 3))).astype(np.float32)
    loc_p = O.w2pers(loc_w, campos, camrot).astype(np.float32)
    vd = rng.normal(size=(n, 3))
    vd = (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)
    params = _weights(kind)
    points = dict(xyz=xyz, emb=emb, color=color, dir=dirs, conf=conf)
    g = O.gather(points, pidx[:, None, :], campos, camrot)

    def run(prm):
        out, rv, _, _ = O.aggregate(prm, g["sampled_color"], None, g["sampled_dir"], g["sampled_conf"],
                                    g["sampled_embedding"], g["sampled_xyz_pers"], g["sampled_xyz"],
                                    g["sample_pnt_mask"], loc_p[:, None, :], loc_w[:, None, :], vd[:, None, :])
        return np.asarray(out)[:, 0], np.asarray(rv)[:, 0]

    ref32, rv = run(params)
    with _oracle_f64():
        ref64, _ = run({k: v.astype(np.float64) for k, v in params.items()})
    assert ref64.dtype == np.float64 and rv.sum() >= n - 1 - (n > EMPTY)
    for a in (xyz, emb, color, dirs, conf, pidx, loc_w, loc_p, vd, ref32, ref64):
        a.setflags(write=False)
    return dict(opt=lego_opt(), points=points, campos=campos, camrot=camrot, pidx=pidx, loc_w=loc_w, loc_p=loc_p,
                vd=vd, params=params, ref32=ref32, ref64=ref64, rv=rv)


def _run_h2(cs, cuda, launches=1):
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints
    pt = cs["points"]
    agg = PointAggregator(cs["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in cs["params"].items()})
    agg.eval()
    np_ = NeuralPoints(cs["opt"], cuda, *(torch.from_numpy(np.array(pt[k])) for k in ("xyz", "emb", "color", "dir", "conf")))
    dev = {k: torch.from_numpy(np.array(cs[k])).to(cuda).contiguous() for k in ("campos", "camrot", "pidx", "loc_w", "loc_p", "vd")}
    n = cs["pidx"].shape[0]
    s = L.Samples(None, None, n, dev["pidx"].data_ptr(), dev["loc_w"].data_ptr(), dev["loc_p"].data_ptr(),
                  dev["vd"].data_ptr(), None, 1, K)
    pts, _keep = np_.tables(dev["campos"], dev["camrot"])
    mlp, _k1 = agg.packed()
    mlph, _k2 = agg.packed_h2()
    outs = []
    for _ in range(launches):
        f = torch.zeros((n, 129), device=cuda)
        scr = L.aggregate_scratch(n, pts.n, cuda)
        L.check(L.lib().pnr_aggregate_fwd_h2(L.ctypes.byref(pts), L.ctypes.byref(s), L.ctypes.byref(mlp),
                                             L.ctypes.byref(mlph), L.ptr(f), None, None, L.ptr(scr), scr.numel() * 4,
                                             L.stream_ptr(cuda)), "pnr_aggregate_fwd_h2")
        outs.append(f)
    torch.cuda.synchronize()
    assert agg.h2_range_ok()
    return [o.cpu().numpy() for o in outs]


def _check(cs, got, what):
    ref64, ref32 = cs["ref64"], cs["ref32"]
    assert got.shape == ref64.shape
    assert not got[~cs["rv"]].any()   # samples without a neighbour stay unwritten
    e32 = np.abs(ref32.astype(np.float64) - ref64)
    eh2 = np.abs(got.astype(np.float64) - ref64)
    scale = np.abs(ref64).max()
    r32, rh2 = np.sqrt((e32 ** 2).mean()), np.sqrt((eh2 ** 2).mean())
    print(f"\n{what}: max|ref| {scale:.3g}  err vs f64 (max, rms): fp32 oracle {e32.max():.3g} {r32:.3g}"
          f"  fp32h2 {eh2.max():.3g} {rh2:.3g}")
    assert eh2.max() <= 2.0 * e32.max() + 1e-7 * scale
    assert rh2 <= 1.5 * r32 + 1e-8 * scale


@pytest.mark.parametrize("n", [5, 2061, 4229])
def test_h2_acc2_sample_counts(cuda, n):
    cs = _case(n, "plain")
    _check(cs, _run_h2(cs, cuda)[0], f"plain n={n}")


def test_h2_acc2_layer_scales(cuda):
    """A wrong 2^s or 2^-11 in the fold shows at once."""
    cs = _case(517, "scales")
    _check(cs, _run_h2(cs, cuda)[0], "scales")


def test_h2_acc2_cancellation(cuda):
    """block1.2's high-half product cancels; the output comes from corr."""
    cs = _case(517, "cancel")
    _check(cs, _run_h2(cs, cuda)[0], "cancel")


def test_h2_acc2_extras_dominate(cuda):
    """block3.0's row group 32 (colour, directions) dominates; three tiles in one
    workgroup catch a stale or early extras write."""
    cs = _case(4229, "extras")
    _check(cs, _run_h2(cs, cuda)[0], "extras")


def test_h2_acc2_deterministic(cuda):
    a, b = _run_h2(_case(2061, "plain"), cuda, launches=2)
    assert np.array_equal(a, b)
