"""The aggregate forward with wide embedding tables (pnr_points.emb_dim 63, 64, 33) and both
agg_intrp_orders (pnr_mlp.intrp_order) against the float64 restatement of
tests/aggregate_dtu_ref.py on hand-built sample lists: pnr_aggregate_fwd, _x3, _h2 with the
f16-split P1 / colour packs (k_point_pre_h2_w, k_tail_o1 on the hid planes), _h2 with them
NULL (k_point_pre_w, k_hid_rows_h2, k_tail_o1 on rows) and _masked, through ctypes the way
tests/test_gpu_aggregate_edges.py calls them (its Dev / run).  DESIGN.md section 31.

Point counts 1, 31, 32, 33, 63, 64, 65, 257 sit on the 32- and 64-point tile edges of the two
per-point kernels; at most 200 sample rows, K = 8; a used subset with a device count below its
capacity; a point exactly at its sample; confidences outside [1e-4, 1]; relu / ReLU weights.
Every output is pre-filled with a canary and carries a canary tail; ALL rows are compared.

Bars, as tests/aggregate_ref.py defines them: the project bar |d| <= 1e-4 + 1e-4 |ref64| and the
tight bar err <= c max(e_o32, 2^-22 max|ref64|) per case and block with c = 8, e_o32 the numpy
fp32 restatement's own error against float64 on the case (CPU, never a kernel's).

Measured on one MI355X (every line in profiles/aggregate_dtu_ratios.txt): see DESIGN.md
section 31 for the worst err / noise ratio of each path and its case.
"""
import os

import numpy as np
import pytest
import torch

import aggregate_dtu_ref as DR
import aggregate_ref as AR
from test_gpu_aggregate_edges import Dev, run

pytestmark = pytest.mark.gpu

C_PATH = {p: DR.C_TIGHT for p in ("fp32", "x3", "h2", "h2_f32colour", "masked")}
SPLIT_PATHS = ("fp32", "x3", "h2", "h2_f32colour")   # h2: with w1ah; h2_f32colour: w1ah (and the colour packs) NULL
WORST = {}
_AGGS = {}


def _opt(E, order, neg_slope=0.01, act_super=1):
    from pointnerf_amd.options import dtu_script_opt
    return dtu_script_opt(point_features_dim=E, agg_intrp_order=order,
                          act_type="LeakyReLU" if neg_slope > 0 else "ReLU", act_super=int(act_super))


def _agg(c, cuda):
    from pointnerf_amd.aggregator import PointAggregator
    key = (c.E, c.order, c.weights, c.neg_slope, c.act_super)
    if key not in _AGGS:
        agg = PointAggregator(_opt(c.E, c.order, c.neg_slope, c.act_super)).to(cuda)
        agg.load_state_dict({k: torch.from_numpy(v) for k, v in DR.case_params(c).items()})
        _AGGS[key] = agg.eval()
    return _AGGS[key]


def _dev(c, cuda, **kw):
    d = Dev(c, cuda, **kw)
    d.pts.emb_dim = c.E
    return d


def _note(path, name, res, e, sc):
    out = {}
    for k, err in res["err"].items():
        noise = max(e[k], AR.ULP_FLOOR * sc[k])
        r = err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))
        out[k] = r
        print(f"RATIO {path:13s} {name:18s} {k:7s} err {err:.3e}  e_o32 {e[k]:.3e}  err/noise {r:8.3f}  "
              f"err/bar {res['bar_ratio'][k]:.5f}")
        w = WORST.setdefault((path, k), [-1.0, name, -1.0, name])
        if r > w[0]:
            w[0], w[1] = r, name
        if res["bar_ratio"][k] > w[2]:
            w[2], w[3] = res["bar_ratio"][k], name
    return out


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nWORST err / max(e_o32, 2^-22 max|ref64|) and err / project bar per path and block")
    for (path, k), (r, rname, b, bname) in sorted(WORST.items()):
        print(f"WORST {path:13s} {k:7s} err/noise {r:8.3f} ({rname})  err/bar {b:.5f} ({bname})")


def _check(path, key, d, agg, masked=False):
    c = d.c
    ref, e, sc = DR.ref64_and_noise(*key, masked=masked)
    got = run(path, d, agg)
    again = run(path, d, agg)
    for a, b in zip(got, again):
        assert np.array_equal(a, b), f"{path} {c.name}: two runs differ"
    res = AR.compare(c, ref, *got)      # every row: written rows against ref64, the others against the canary
    assert not res["canary"], (path, c.name, res["canary"])
    ratios = _note(path, c.name, res, e, sc)
    fails = [(k, res["bar_ratio"][k]) for k in ratios if res["bar_ratio"][k] > 1.0]
    assert not fails, f"{path} {c.name}: over the project bar {fails}"
    tight = [(k, r) for k, r in ratios.items() if r > C_PATH[path]]
    assert not tight, f"{path} {c.name}: err / max(e_o32, 2^-22 max|ref|) over c = {C_PATH[path]}: {tight}"


@pytest.mark.parametrize("base, E, order", DR.CASES)
def test_wide_paths_vs_fp64(cuda, base, E, order):
    """fp32, x3, h2 with w1ah, h2 with w1ah NULL: canaries, both bars, two runs bitwise equal, range flag."""
    c = DR.case(base, E, order)
    d, agg = _dev(c, cuda), _agg(c, cuda)
    for path in SPLIT_PATHS:
        _check(path, (base, E, order), d, agg)


@pytest.mark.parametrize("base, E, order", [k for k in DR.CASES if k[0] in DR.MASKED_OK])
def test_wide_masked_vs_fp64(cuda, base, E, order):
    """pnr_aggregate_fwd_masked on the pair-table twin of the case."""
    c = DR.masked_case(base, E, order)
    _check("masked", (base, E, order), _dev(c, cuda), _agg(c, cuda), masked=True)


@pytest.mark.parametrize("path", ["fp32", "h2"])
def test_used_subset_equals_full_table_wide(cuda, path):
    c = DR.case("used", 63, 1)
    agg = _agg(c, cuda)
    a = run(path, _dev(c, cuda, use_used=True), agg)
    b = run(path, _dev(c, cuda, use_used=False), agg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_h2_point_pre_then_p1_ready_wide(cuda):
    """pnr_point_pre_h2 at emb_dim 63 into the scratch, then the h2 call with p1_ready = 1, equals the one call."""
    from pointnerf_amd import _lib as L
    c = DR.case("n65", 63, 1)
    d, agg = _dev(c, cuda), _agg(c, cuda)
    one = run("h2", d, agg)
    scr = d.scratch()
    mh, _keep = agg.packed_h2()
    L.check(L.lib().pnr_point_pre_h2(L.ctypes.byref(d.pts), L.ctypes.byref(mh), L.ptr(scr), scr.numel() * 4,
                                     L.stream_ptr(cuda)), "pnr_point_pre_h2")
    two = run("h2", d, agg, scr=scr, p1_ready=1)
    for x, y in zip(one, two):
        assert np.array_equal(x, y)


def test_order_is_the_only_difference_between_the_two_tails(cuda):
    """Order 1 against order 2 on one case: weights and confidences equal bit for bit, the same rows written,
    the colours raw2out_color of order 2's."""
    c2, c1 = DR.case("n33", 63, 2), DR.case("n33", 63, 1)
    f2, w2, cf2 = run("fp32", _dev(c2, cuda), _agg(c2, cuda))
    f1, w1, cf1 = run("fp32", _dev(c1, cuda), _agg(c1, cuda))
    assert np.array_equal(w1, w2) and np.array_equal(cf1, cf2)
    wr = f2[:, 0] != AR.CANARY_FEAT
    assert np.array_equal(wr, f1[:, 0] != AR.CANARY_FEAT) and wr.any()
    sig = 1.0 / (1.0 + np.exp(-f2[wr, 1:].astype(np.float64)))
    np.testing.assert_allclose(f1[wr, 1:], sig * 1.002 - 0.001, atol=2e-6, rtol=0)


# ------------------------------------------------------------------ the reference's own outputs
@pytest.mark.parametrize("pre, E, order", [("a_", 63, 2), ("a_", 63, 1), ("b_", 32, 1)])
def test_forward_matches_reference_fixture(cuda, golden_dir, pre, E, order):
    """The fixture's gathered inputs through PointAggregator.forward (the masked path) against the reference
    PointAggregator's recorded outputs, to the project bar."""
    from pointnerf_amd.aggregator import PointAggregator
    g = np.load(os.path.join(golden_dir, "aggregator_dtu.npz"), allow_pickle=False)
    agg = PointAggregator(_opt(E, order)).to(cuda).eval()
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in DR.params_for(E, float(g["salt"])).items()})
    t = {k: torch.from_numpy(g[pre + k]).to(cuda) for k in
         ("sampled_color", "sampled_dir", "sampled_conf", "sampled_embedding", "sampled_xyz_pers", "sampled_xyz",
          "sample_pnt_mask", "sample_loc", "sample_loc_w", "sample_ray_dirs")}
    with torch.no_grad():
        feats, ray_valid, weight, conf = agg(t["sampled_color"], torch.eye(3, device=cuda), t["sampled_dir"],
                                             t["sampled_conf"], t["sampled_embedding"], t["sampled_xyz_pers"],
                                             t["sampled_xyz"], t["sample_pnt_mask"], t["sample_loc"],
                                             t["sample_loc_w"], t["sample_ray_dirs"], [0.004, 0.004, 0.004], 0)
    want = g[f"{pre}features_o{order}"]
    assert np.array_equal(ray_valid.cpu().numpy(), g[pre + "ray_valid"])
    got = feats.cpu().numpy()
    d = np.abs(got.astype(np.float64) - want)
    print(f"fixture {pre} E{E} order {order}: max |d| {d.max():.3e}, max |d| / bar {(d / (AR.ATOL + AR.RTOL * np.abs(want))).max():.4f}")
    assert np.all(d <= AR.ATOL + AR.RTOL * np.abs(want))
    assert np.all(got[~g[pre + "ray_valid"]] == 0)
    np.testing.assert_allclose(weight.cpu().numpy(), g[pre + "weight"], atol=AR.ATOL, rtol=AR.RTOL)
    np.testing.assert_allclose(conf.cpu().numpy(), g[pre + "conf_coefficient"], atol=1e-7, rtol=0)
