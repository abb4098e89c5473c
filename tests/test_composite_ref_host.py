"""CPU checks of tests/composite_ref.py: the generator's invariants, the
restatement pinned to ``oracle.render`` on a real query, and -- for every case
tests/test_gpu_composite.py runs -- the fp32 restatement inside the GPU test's
tolerance against the fp64 one (the bar can be met by correct fp32 arithmetic).
"""
import numpy as np
import pytest
import torch

import composite_ref as CR
from formula import formula_params
from oracle import oracle as O
from scenes import oracle_points, scene


def _rays(b):
    n, off = b["n_filled"].numpy(), b["ray_off"].numpy()
    vflag, z = b["vflag"].numpy(), b["sample_p"].numpy()[:, 2]
    for r in range(b["R"]):
        yield r, n[r], vflag[off[r]:off[r] + n[r]], z[off[r]:off[r] + n[r]]


def check_bufs(b, n_cams=1):
    """The scan relations of the buffers and every forced pattern; run on the very
    buffers of each GPU case, so the upper half cannot go empty unnoticed."""
    R, SR = b["R"], b["SR"]
    n, vflag, vcnt = b["n_filled"].numpy(), b["vflag"].numpy(), b["ray_vcnt"].numpy()
    assert (n >= 0).all() and (n <= SR).all()
    assert np.array_equal(b["ray_off"].numpy(), np.concatenate([[0], np.cumsum(n)]))
    assert b["S"] == n.sum() == vflag.shape[0] and set(np.unique(vflag)) <= {0, 1}
    assert np.array_equal(b["valid_off"].numpy(), np.concatenate([[0], np.cumsum(vflag)]))
    assert np.array_equal(vcnt, [v.sum() for _, _, v, _ in _rays(b)])
    assert np.array_equal(b["ray_row"].numpy(), np.concatenate([[0], np.cumsum(vcnt > 0)]))
    assert b["S_valid"] == vflag.sum() and b["R_valid"] == (vcnt > 0).sum()
    assert b["sample_p"].shape == (b["S"], 3) and b["pidx"].shape == (b["S"], b["K"])
    assert (b["pidx"].numpy() < b["xyz"].shape[0]).all() and (b["pidx"].numpy() >= -1).all()
    if n_cams > 1:
        assert set(b["ray_cam"].numpy()) == set(range(n_cams))
        assert len(set(CR.origin_depth(b["campos"].numpy(), b["camrot"].numpy()))) == n_cams
    # every forced pattern is present
    for want in {0, 1, 63, 64, 65, SR - 1, SR}:
        if 0 <= want <= SR:
            assert (n == want).any(), f"no ray with n_filled = {want}"
    rays = list(_rays(b))
    assert any(k == SR and v[0] and v.sum() == 1 for _, k, v, _ in rays), "valid only at slot 0"
    assert any(k == SR and v[SR - 1] and v.sum() == 1 for _, k, v, _ in rays), "valid only at slot SR - 1"
    assert any(k > 0 and v.sum() == 0 for _, k, v, _ in rays), "filled but none valid"
    assert vcnt[b["names"]["none_valid"]] == 0 and n[b["names"]["none_valid"]] > 0
    if SR > 8:
        assert (vcnt > 8).any()
    if SR > 64:
        assert (vcnt > 64).any()
        # the gap this suite closes: valid data at slot index >= 64, and a ray with nothing below it
        assert CR.upper_half_valid(b)
        assert any(k > 64 and not v[:64].any() and v[64:].any() for _, k, v, _ in rays), "valid only at index >= 64"
    if SR >= 12:
        zo = CR.origin_depth(b["campos"].numpy(), b["camrot"].numpy())
        cam = b["ray_cam"].numpy() if n_cams > 1 else np.zeros(R, int)
        d = [np.diff(z) for _, _, _, z in rays]
        assert any((x < 0).any() for x in d), "non-monotone z"
        assert any((x == 0).any() for x in d), "equal neighbouring depths"
        assert any((x > np.float32(2 * CR.VSIZE_Z)).any() for x in d), "gap above 2 vsize_z"
        assert any(k and (z < zo[cam[r]]).all() for r, k, _, z in rays), "all samples below the origin depth"
        assert any(k and (z > zo[cam[r]]).all() for r, k, _, z in rays), "all samples above the origin depth"
        assert any(k and (z < zo[cam[r]]).any() and (z > zo[cam[r]]).any() for r, k, _, z in rays)
    # the distance rules really fire on the scattered buffers, for both unit modes
    loc, rv, _ = CR.scatter_dense(b, None)
    if SR >= 12:
        cm = np.maximum.accumulate(loc[..., 2], -1)
        raw = cm[:, 1:] - cm[:, :-1]
        assert (raw[rv[:, :-1]] < np.float32(1e-8)).any() and (raw[rv[:, :-1]] > np.float32(2 * CR.VSIZE_Z)).any()
        d1, d0 = O.ray_dist(loc, rv, CR.VSIZE_Z, 1), O.ray_dist(loc, rv, CR.VSIZE_Z, 0)
        assert (d1 != d0).any() and d1.max() <= np.float32(2 * CR.VSIZE_Z) < d0.max()


@pytest.mark.parametrize("n_cams", [1, 3])
@pytest.mark.parametrize("SR", sorted(set(CR.FUSED_SR)))
def test_generator_invariants(SR, n_cams):
    check_bufs(CR.make_bufs(CR.FUSED_R, SR, seed=SR, n_cams=n_cams), n_cams)


def test_cases_cover_the_lists():
    for cases, srs, cs in ((CR.DENSE_CASES, CR.DENSE_SR, CR.DENSE_C), (CR.FUSED_CASES, CR.FUSED_SR, CR.FUSED_C)):
        for bg in (True, False):
            assert {c[0] for c in cases if c[2] == bg} == set(srs)
            assert {c[1] for c in cases if c[2] == bg} == set(cs)
    for unit in (0, 1):
        assert {c[0] for c in CR.FUSED_CASES if c[3] == unit} == set(CR.FUSED_SR)
    assert {c[1] for c in CR.FUSED_HF_CASES} == {c for c in CR.FUSED_C if c % 2 == 0}
    assert {c[0] for c in CR.FUSED_HF_CASES} == set(CR.FUSED_SR)
    # dense fixed rays: the upper-half-only ray exists whenever SR > 64
    for SR, C, _ in CR.DENSE_CASES:
        d = CR.make_dense(CR.DENSE_NR, SR, C, seed=CR.case_seed(SR, C))
        rv = d["rv"].numpy()
        assert not rv[d["fixed"]["all_invalid"]].any()
        assert rv[d["fixed"]["only_slot0"]].sum() == 1 and rv[d["fixed"]["only_slot0"], 0]
        assert rv[d["fixed"]["only_last"]].sum() == 1 and rv[d["fixed"]["only_last"], SR - 1]
        if SR > 64:
            u = d["fixed"]["upper_only"]
            assert not rv[u, :64].any() and rv[u, 64:].all()
            assert rv[4:, 64:].any() and rv[4:, :64].any()   # and random rays valid in both halves


def test_hf_rows_round_trip():
    b = CR.make_bufs(CR.FUSED_R, 65, seed=1)
    f = CR.make_feat(b, 66, seed=1, bf16=True)
    rows = CR.pack_hf(f)
    assert rows.shape == (b["S_valid"], CR.FEAT_H_PITCH) and rows.dtype == torch.int16
    assert torch.equal(CR.unpack_hf(rows, b["S_valid"], 66), f)


def test_restatement_reproduces_oracle_render():
    """oracle.render's query and features as buffers -> composite_reference in
    fp32.  ray_dist comes from the same numpy fp32 function on the same values and
    ray_mask / the background rays are copies: np.array_equal.  Colour, opacity
    and is_bg go through torch fp32 (exp, cumprod, sum) instead of numpy fp32:
    within 1e-6."""
    sc = scene(8000, H=24, W=24, theta=40.0)
    opt = sc["opt"]
    ref = O.render(opt, oracle_points(sc), formula_params(salt=0.25), sc["campos"], sc["camrot"], sc["raydir"],
                   sc["bg"])
    q, rv, feats = ref["query"], ref["ray_valid"], ref["features"]
    mask = q["ray_mask"] > 0
    R, SR, K = mask.shape[0], opt.SR, opt.K
    filled = (q["sample_loc_w"] != 0).any(-1)            # [R'',SR]
    assert not (rv & ~filled).any()
    nf = filled.sum(-1)
    assert all(filled[i, :nf[i]].all() for i in range(filled.shape[0]))   # filled slots come first
    n_filled = np.zeros(R, np.int32)
    n_filled[mask] = nf
    vflag = rv[filled].astype(np.int32)
    vcnt = np.zeros(R, np.int32)
    vcnt[mask] = rv.sum(-1)
    t = torch.from_numpy
    b = dict(R=R, SR=SR, K=K, S=int(nf.sum()), S_valid=int(vflag.sum()), R_valid=int(mask.sum()),
             n_filled=t(n_filled), ray_off=t(np.concatenate([[0], np.cumsum(n_filled)]).astype(np.int32)),
             vflag=t(vflag), valid_off=t(np.concatenate([[0], np.cumsum(vflag)]).astype(np.int32)),
             ray_vcnt=t(vcnt), ray_row=t(np.concatenate([[0], np.cumsum(vcnt > 0)]).astype(np.int32)),
             sample_p=t(np.ascontiguousarray(q["sample_loc"][filled])), ray_cam=None,
             campos=t(sc["campos"].reshape(1, 3)), camrot=t(sc["camrot"].reshape(1, 3, 3)))
    assert (vcnt[mask] > 0).all() and b["S_valid"] > 50
    feat = t(np.ascontiguousarray(feats[rv]))
    params = dict(vsize_z=opt.vsize[2], unit=opt.raydist_mode_unit, bg=t(sc["bg"]), feat_rows=0)
    got = CR.composite_reference(b, feat, None, params, torch.float32)
    assert np.array_equal(got["ray_dist"][mask], ref["ray_dist"])
    assert np.array_equal(got["ray_mask"].numpy(), ref["ray_mask"])
    c, o, ib = got["ray_color"].numpy(), got["opacity"].numpy(), got["is_bg"].numpy()
    assert np.array_equal(c[~mask], ref["coarse_raycolor"][~mask])
    assert np.array_equal(o[~mask], ref["coarse_point_opacity"][~mask]) and (ib[~mask] == 1).all()
    assert np.abs(c - ref["coarse_raycolor"]).max() <= 1e-6
    assert np.abs(o - ref["coarse_point_opacity"]).max() <= 1e-6
    assert np.abs(ib - ref["coarse_is_background"][:, 0]).max() <= 1e-6
    # the explicit cams argument is the buffers' own camera
    got2 = CR.composite_reference(b, feat, (sc["campos"], sc["camrot"]), params, torch.float32)
    assert torch.equal(got2["ray_color"], got["ray_color"])


ALL5 = ("color", "opacity", "acc_T", "blend", "bgT")
ABS = {"bgT": CR.TINY, "is_bg": CR.TINY, "d_bg": CR.TINY}


def _dense_fp32_vs_fp64(NR, SR, C, bg, sat=False, seed=0):
    d = CR.make_dense(NR, SR, C, seed=seed, sat=sat)
    g = CR.dense_grads(NR, SR, C, seed=seed)
    bgc = d["bg"] if bg else None
    w = CR.Worst()
    for grads in (dict(color=g["color"]), g):
        a = CR.march_reference(d["rd"], d["rv"], d["rf"], bgc, torch.float32, grads)
        r = CR.march_reference(d["rd"], d["rv"], d["rf"], bgc, torch.float64, grads)
        for k in ALL5 + ("d_feat", "d_dist") + (("d_bg",) if bg else ()):
            assert torch.isfinite(a[k]).all()
            w.close(a[k], r[k], k, ABS.get(k, 0.0), what=f"fp32 restatement SR={SR} C={C}")
    return w.w


@pytest.mark.parametrize("SR,C,bg", CR.DENSE_CASES)
def test_fp32_restatement_meets_bar_dense(SR, C, bg):
    _dense_fp32_vs_fp64(CR.DENSE_NR, SR, C, bg, seed=CR.case_seed(SR, C))


@pytest.mark.parametrize("SR,C", [(128, 3), (65, 64)])
def test_fp32_restatement_meets_bar_dense_saturated(SR, C):
    _dense_fp32_vs_fp64(CR.DENSE_NR, SR, C, True, sat=True, seed=CR.case_seed(SR, C))


def test_fp32_restatement_meets_bar_dense_grid_stride_and_wrapper():
    _dense_fp32_vs_fp64(16384 + 37, 2, 3, True, seed=5)
    w = CR.WRAPPER_CASE
    _dense_fp32_vs_fp64(w["B"] * w["R"], w["SR"], w["C"], True, seed=w["seed"])


def _fused_fp32_vs_fp64(b, C, bg, unit, feat_rows=0, seed=0, bf16=False):
    feat = CR.make_feat(b, C, seed=seed, bf16=bf16)
    g = torch.Generator().manual_seed(4000 + seed)
    d_color = torch.randn((b["R"], C), generator=g)
    params = dict(vsize_z=CR.VSIZE_Z, unit=unit, bg=torch.rand(C, generator=g) if bg else None, feat_rows=feat_rows)
    a = CR.composite_reference(b, feat, None, params, torch.float32, d_color)
    r = CR.composite_reference(b, feat, None, params, torch.float64, d_color)
    assert torch.equal(a["ray_mask"], r["ray_mask"])
    w = CR.Worst()
    for k in ("ray_color", "opacity", "is_bg", "blend", "d_feat"):
        assert torch.isfinite(a[k]).all()
        w.close(a[k], r[k], k, ABS.get(k, 0.0), what=f"fp32 restatement SR={b['SR']} C={C}")


@pytest.mark.parametrize("SR,C,bg,unit", CR.FUSED_CASES)
def test_fp32_restatement_meets_bar_fused(SR, C, bg, unit):
    b = CR.make_bufs(CR.FUSED_R, SR, seed=CR.case_seed(SR, C))
    check_bufs(b)
    _fused_fp32_vs_fp64(b, C, bg, unit, seed=CR.case_seed(SR, C), bf16=C % 2 == 0)


def test_fp32_restatement_meets_bar_fused_special():
    b = CR.make_bufs(CR.FUSED_R, 128, seed=77, n_cams=3)
    check_bufs(b, 3)
    _fused_fp32_vs_fp64(b, 66, True, 1, seed=77)
    _fused_fp32_vs_fp64(b, 66, False, 0, seed=77)
    b = CR.make_bufs(CR.FUSED_R, 80, seed=78)
    check_bufs(b)
    _fused_fp32_vs_fp64(b, 128, True, 1, feat_rows=b["S_valid"] - 7, seed=78)
    b = CR.make_bufs(16384 + 37, 2, seed=79, forced=False)
    _fused_fp32_vs_fp64(b, 3, True, 1, seed=79)
    c = CR.ROW_CAP_CASE
    b = CR.make_bufs(CR.FUSED_R, c["SR"], K=c["K"], seed=c["seed"])
    check_bufs(b)
    _fused_fp32_vs_fp64(b, c["C"], True, 1, seed=c["seed"])


def _dense_errs(SR, C, bg, drop, seed):
    """err / tol per tensor of the emulated two-half algorithm (all five output
    gradients) against the fp64 restatement, on the GPU test's own inputs."""
    d = CR.make_dense(CR.DENSE_NR, SR, C, seed=seed)
    g = CR.dense_grads(CR.DENSE_NR, SR, C, seed=seed)
    bgc = d["bg"] if bg else None
    r = CR.march_reference(d["rd"], d["rv"], d["rf"], bgc, torch.float64, g)
    e = CR.two_half_march(d["rd"], d["rv"], d["rf"], bgc, g, drop=drop)
    return {k: CR.err_over_tol(e[k], r[k], ABS.get(k, 0.0)) for k in e if e[k] is not None}


@pytest.mark.parametrize("SR,C,bg", CR.DENSE_CASES)
def test_two_half_emulation_is_the_restatement(SR, C, bg):
    errs = _dense_errs(SR, C, bg, None, CR.case_seed(SR, C))
    assert max(errs.values()) < 1e-6, errs   # fp64 on both sides


@pytest.mark.parametrize("drop", CR.HANDOVERS_MARCH)
def test_dense_cases_catch_a_dropped_handover(drop):
    """Each upper-half hand-over of march_slots / march_slots_bwd, left out of the
    emulation, misses the GPU test's bar more than tenfold on every dense case with
    SR > 64 (and changes nothing at SR <= 64, which is why the gap stayed open)."""
    for SR, C, bg in CR.DENSE_CASES:
        worst = max(_dense_errs(SR, C, bg, drop, CR.case_seed(SR, C)).values())
        if SR > 64:
            assert worst > 10.0, (drop, SR, C, bg, worst)
        elif drop != "e1":   # "e1" puts lane 0's own product where tot0 belongs: visible in no output at SR <= 64
            assert worst < 1e-6, (drop, SR, C, bg, worst)


@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("SR", sorted(set(CR.FUSED_SR)))
def test_fused_cases_catch_a_dropped_depth_handover(SR, unit):
    b = CR.make_bufs(CR.FUSED_R, SR, seed=SR)
    loc, rv, _ = CR.scatter_dense(b, None)
    ref = O.ray_dist(loc, rv, CR.VSIZE_Z, unit)
    assert np.array_equal(CR.two_half_dist(loc, rv, CR.VSIZE_Z, unit), ref)
    for drop in CR.HANDOVERS_DIST:
        got = CR.two_half_dist(loc, rv, CR.VSIZE_Z, unit, drop=drop)
        if SR == 65 and drop == "cm0":
            # slot 64 is the last one (distance vsize_z) and slot 63's difference is clamped to
            # vsize_z either way: the carried maximum shows only from two upper slots on
            assert np.array_equal(got, ref)
        elif SR > 64:
            # a distance off by more than 10 % of vsize_z on a valid slot: far outside the bar on opacity
            assert np.abs(got - ref).max() > 0.1 * CR.VSIZE_Z, (drop, SR)
        else:
            assert np.array_equal(got, ref)


@pytest.mark.parametrize("SR,K", CR.AUX_CASES)
def test_fp32_restatement_meets_bar_aux_weight(SR, K):
    b = CR.make_bufs(CR.FUSED_R, SR, K=K, seed=SR + K)
    check_bufs(b)
    e = CR.Worst().close(CR.aux_weight_reference(b, torch.float32), CR.aux_weight_reference(b), "weight",
                         what=f"fp32 restatement SR={SR} K={K}")
    assert e < 0.1


def test_aux_weight_reference_properties():
    b = CR.make_bufs(CR.FUSED_R, 65, K=8, seed=3)
    w = CR.aux_weight_reference(b)
    assert w.shape == (b["R_valid"], 65, 8) and (w >= 0).all()
    s = w.sum(-1)
    assert ((s - 1).abs() < 1e-12).logical_or(s == 0).all() and (s == 0).any() and (s > 0).any()
