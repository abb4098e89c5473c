"""CPU checks of tests/aggregate_train_ref.py, the pinned-sign restatement the GPU
suite tests/test_gpu_aggregate_train.py compares the training kernels with.

With its own signs, in float64: its feat is aggregate_ref.reference's and its
gradients are torch autograd of oracle_grad.aggregate on the same gathered inputs;
it reproduces the reference project's own autograd gradients
(tests/golden/aggregator_bwd.npz) under the tolerance of
test_aggregator_bwd_vs_reference_golden.  Each emulated backward bug fails a named
case on a named gradient tensor by more than ten times that tensor's tight bar
(c = 8) while the clean float32 run stays under it.  Pinning is harmless on the
reference alone: with the float32 run's signs forced on the float64 run, every
entry whose sign differs has |z64| within the tight bar of its layer.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aggregate_ref as AR
import aggregate_train_ref as TR
from formula import formula_params
from oracle import oracle_grad as OG

F32 = np.float32


def _rel(a, b):
    s = float(np.abs(b).max())
    d = float(np.abs(np.asarray(a, np.float64) - b).max()) if np.size(b) else 0.0
    return d / s if s > 0 else d


@pytest.mark.parametrize("name", AR.SMALL)
def test_feat_is_the_forward_reference(name):
    """signs=None, float64: feat == aggregate_ref.reference(case, float64) to 1e-12 relative,
    the same rows untouched."""
    c = AR.case(name)
    want = AR.reference(c, np.float64)
    got = TR.reference(c, np.float64)
    assert np.array_equal(got["untouched"], want["untouched"])
    assert got["feat"].shape == want["feat"].shape
    assert _rel(got["feat"], want["feat"]) <= 1e-12, _rel(got["feat"], want["feat"])
    assert not got["feat"][got["untouched"]].any()


def _oracle_grads(c, xyz_grad):
    """torch autograd of oracle_grad.aggregate (float64) on the inputs gathered as
    aggregate_ref.reference gathers them, <G, feat> with TR.upstream."""
    gi = TR.gather_indices(c)
    n, K = gi.n, c.K
    t64 = lambda a: torch.from_numpy(np.array(a)).double()   # noqa: E731
    idx = torch.from_numpy(gi.idx)
    leaf = {k: t64(getattr(c, k)).requires_grad_(True) for k in ("emb", "color", "dir", "conf")
            if getattr(c, k) is not None}
    xyz = t64(c.xyz).requires_grad_(xyz_grad)
    pp = {k: t64(v).requires_grad_(True) for k, v in AR.params_of(c).items()}
    xyz_g = xyz[idx]
    if c.pers is not None:
        pers_g = t64(c.pers)[idx]
    else:
        parts = []
        for ci in range(c.campos.shape[0]):
            parts.append(TR._w2pers(xyz_g, t64(c.campos[ci]), t64(c.camrot[ci])))
        sel = torch.from_numpy(gi.cam)[:, None, None].expand(n, K, 3)
        pers_g = parts[0] if len(parts) == 1 else torch.where(sel == 0, parts[0], parts[1])
    z3 = torch.zeros((n, K, 3), dtype=torch.float64)
    if c.rw2c is not None:
        rw = t64(c.rw2c).reshape(-1, 3, 3)[idx][:, None]
    else:
        rw = None if c.Rw2c is None else t64(c.Rw2c)
    s = lambda a: a[:, None]   # noqa: E731
    feat, rv, _, _ = OG.aggregate(pp, s(leaf["color"][idx] if "color" in leaf else z3),
                                  s(leaf["dir"][idx] if "dir" in leaf else z3),
                                  s(leaf["conf"][idx][..., None]) if "conf" in leaf else None, s(leaf["emb"][idx]),
                                  s(pers_g), s(xyz_g), s(torch.from_numpy(gi.mask)), s(t64(c.sample_p[gi.rows])),
                                  s(t64(c.sample_w[gi.rows])), s(t64(c.dirs[gi.drow])), rw2c=rw,
                                  neg_slope=c.neg_slope, act_super=c.act_super)
    G = torch.from_numpy(TR.upstream(c))[:n]
    (feat[:, 0] * G).sum().backward()
    if xyz_grad:
        leaf["xyz"] = xyz
    g = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in {**leaf, **pp}.items()}
    return g


@pytest.mark.parametrize("name", AR.SMALL)
def test_gradients_are_oracle_grad_autograd(name):
    """signs=None, float64: every point and parameter gradient (d xyz too, except on
    pers_given) equals torch autograd of oracle_grad.aggregate to 1e-10 relative."""
    c = AR.case(name)
    xg = c.pers is None
    got = TR.reference(c, np.float64, xyz_grad=xg)
    if got["n"] == 0:
        assert all(not g.any() for g in got["grads"].values())
        return
    want = _oracle_grads(c, xg)
    for k, w in want.items():
        assert np.isfinite(got["grads"][k]).all(), k
        assert _rel(got["grads"][k], w) <= 1e-10, (name, k, _rel(got["grads"][k], w))


def _golden_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "aggregator.npz"), allow_pickle=False)
    gb = np.load(os.path.join(golden_dir, "aggregator_bwd.npz"), allow_pickle=False)
    _, R, SR, K = g["sample_pnt_mask"].shape
    rows = R * SR
    flat = lambda k, ch: np.ascontiguousarray(g[k].reshape(rows * K, ch))   # noqa: E731
    c = SimpleNamespace(
        name="golden", N=rows * K, K=K, rows=rows, xyz=flat("sampled_xyz", 3), emb=flat("sampled_embedding", 32),
        color=flat("sampled_color", 3), dir=flat("sampled_dir", 3), conf=flat("sampled_conf", 1)[:, 0],
        pers=flat("sampled_xyz_pers", 3), rw2c=None, Rw2c=None, campos=np.zeros((1, 3), F32),
        camrot=np.eye(3, dtype=F32)[None], ray_cam=None, pidx=None,
        pair_mask=g["sample_pnt_mask"].reshape(-1).astype(np.uint8), sample_w=g["sample_loc_w"].reshape(rows, 3),
        sample_p=g["sample_loc"].reshape(rows, 3), dirs=g["sample_ray_dirs"].reshape(rows, 3), dir_map=None,
        dir_div=1, samp_list=None, n_max=rows, n_dev=rows, used=None, used_map=None, n_used_dev=None,
        neg_slope=0.01, act_super=1, weights=("formula", 0.0), edges={})
    return c, g, gb


def _close(a, ref, name, rel=1e-4, scale=1e-5):
    """test_gpu_backward.close: |d| <= scale max|ref| + rel |ref|."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    tol = scale * max(float(np.abs(ref).max()), 1e-30) + rel * np.abs(ref)
    bad = np.abs(a - ref) > tol
    assert not bad.any(), f"{name}: {bad.sum()} / {bad.size} outside tol, max |d| {np.abs(a - ref).max():.3e}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_reproduces_the_reference_projects_autograd(golden_dir, dtype):
    """aggregator.npz + formula_params() -> aggregator_bwd.npz (the reference project's own
    autograd), under test_aggregator_bwd_vs_reference_golden's tolerance."""
    c, g, gb = _golden_case(golden_dir)
    r = TR.reference(c, dtype, G=gb["g_feat"].reshape(c.rows, 129).astype(np.float64), params=formula_params())
    _close(r["feat"], gb["features"].reshape(c.rows, 129), "features")
    for k, gk in (("color", "g_sampled_color"), ("dir", "g_sampled_dir"), ("conf", "g_sampled_conf"),
                  ("emb", "g_sampled_embedding")):
        _close(r["grads"][k].reshape(gb[gk].shape), gb[gk], "d " + k)
    for k in TR.PARAM_NAMES:
        _close(r["grads"][k], gb["gp_" + k.replace(".", "_")], "d " + k)


# mutation -> (case, the tensor it must show on, xyz_grad)
MUT_CASES = {
    "mask_words_swapped": ("count_9", "block1.2.weight", False),
    "empty_dz_kept": ("K_3", "block3.2.weight", False),
    "skip_last_tile": ("count_9", "emb", False),
    "conf_clamp_derivative": ("conf_range", "conf", False),
    "dir_no_rwT": ("rw2c_point", "dir", False),
    "xyz_no_dS": ("count_9", "xyz", True),
    "xyz_cam0": ("two_cams", "xyz", True),
    "ignore_used_map": ("used_subset", "emb", False),
    "ignore_n_dev": ("ndev_37", "block3.2.weight", False),
}


def test_every_mutation_has_a_case():
    assert set(MUT_CASES) == set(TR.MUTATIONS) and len(TR.MUTATIONS) >= 8


def test_mutations_fail_their_cases_by_ten_times_the_tight_bar():
    """Each emulated backward bug, applied to the float64 gradient under the clean run's
    signs, is more than 10 x over the tight bar (c = 8) of its tensor on its case; the
    clean float32 run is under that bar on every tensor of that case.  That second half is an
    identity, printed for the table and no check of anything: e_o32 IS the float32 run's error,
    so e / (8 max(e, floor)) <= 1 / 8 by construction.  The mutation half is the check."""
    print(f"\n{'mutation':24s} {'case':12s} {'tensor':18s} {'err':>10s} {'bar(c=8)':>10s} {'err/bar':>9s} "
          f"{'clean32/bar':>11s}")
    bad = []
    for mut, (name, tensor, xg) in MUT_CASES.items():
        c = AR.case(name)
        r64, e, sc = TR.noise(c, xyz_grad=xg)
        m = TR.reference(c, np.float64, r64["signs"], xg, mut=mut)
        clean = max(e[k] / TR.tight_bar(e[k], sc[k]) for k in r64["grads"] if sc[k] > 0)
        bar = TR.tight_bar(e[tensor], sc[tensor])
        err = float(np.abs(m["grads"][tensor] - r64["grads"][tensor]).max())
        print(f"{mut:24s} {name:12s} {tensor:18s} {err:10.3e} {bar:10.3e} {err / bar:9.1f} {clean:11.3f}")
        if not (err > 10 * bar and clean <= 1.0):
            bad.append((mut, name, tensor, err / bar, clean))
    assert not bad, bad


@pytest.mark.parametrize("name", AR.SMALL)
def test_pinning_is_harmless_on_the_reference(name):
    """The float32 run's signs forced on the float64 run: every entry whose sign differs
    from z64 > 0 has |z64| <= C_TIGHT max(e_o32(layer), 2^-22 max|z64(layer)|) -- the
    condition the GPU suite puts on the kernel's saved signs."""
    c = AR.case(name)
    r64, e, sc = TR.noise(c)
    if r64["n"] == 0:
        return
    r32 = TR.reference(c, np.float32)           # its own signs
    pinned = TR.reference(c, np.float64, r32["signs"])
    tot = dis = 0
    for k in TR.SIGN_KEYS:
        if k == "pa" and c.act_super:
            continue
        live = r64["mask"] if k.startswith("h") and not k.startswith("hc") or k == "pa" else ~r64["untouched"][:r64["n"]]
        z64 = pinned["z"][k][live]
        d = (r32["signs"][k][live] != (z64 > 0))
        bar = TR.tight_bar(e["z:" + k], sc["z:" + k])
        tot += d.size
        dis += int(d.sum())
        assert not d.any() or np.abs(z64[d]).max() <= bar, (name, k, float(np.abs(z64[d]).max()), bar)
    print(f"SIGNS {name:18s} {dis} of {tot} entries disagree ({dis / max(tot, 1):.2e})")
