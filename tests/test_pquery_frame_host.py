"""CPU checks of the fused perspective frame's test infrastructure (DESIGN.md 29,
tests/pquery_frame_ref.py): the scenes still hold what the GPU tests rely on,
the expected query buffers are self-consistent on every scene and pixel subset,
and correct fp32 arithmetic meets the composite cases' tolerance in the
perspective mode (as test_composite_ref_host.py shows for the world mode)."""
import numpy as np
import pytest
import torch

import composite_ref as CR
import pquery_frame_ref as FR

ABS = {"is_bg": CR.TINY}


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in "ABC":
        sc = FR.scene(name)
        out[name] = (sc, FR.ref_query(sc))
    return out


def _bufs(sc, q):
    return FR.expected_from_query(q, int(sc["opt"].SR), int(sc["opt"].K))


def test_scene_a_has_neighbourless_rays_and_saturated_columns(scenes):
    sc, q = scenes["A"]
    e = _bufs(sc, q)
    # the lone point's block adds 36 hit rays to the base scene's 976
    assert len(q["ray_mask"]) == FR.SCENE_R and int(q["ray_mask"].sum()) == FR.SCENE_HIT["A"] == 976 + 36
    assert int(((e["ray_hit"] != 0) & (e["ray_vcnt"] == 0)).sum()) == 134 >= 130   # hit rays without any neighbour
    assert int((e["vflag"] == 0).sum()) == 5176                                 # filled samples without a neighbour
    assert int((e["n_filled"] == sc["opt"].SR).sum()) == 516                    # rays saturated at SR 24
    nn = (e["pidx"] >= 0).sum(1)
    assert int(((nn >= 1) & (nn <= 7)).sum()) == 9972                           # partly filled neighbour lists


def test_scene_b_reaches_the_second_lane_half(scenes):
    sc, q = scenes["B"]
    e = _bufs(sc, q)
    assert len(q["ray_mask"]) == FR.SCENE_R and int(q["ray_mask"].sum()) == FR.SCENE_HIT["B"]
    assert int((e["n_filled"] > 64).sum()) == 552
    assert int((e["n_filled"] == 80).sum()) == 508
    assert int((e["vflag"] == 0).sum()) == 13544


def test_scene_c_truncates_columns_at_sr(scenes):
    sc, q = scenes["C"]
    assert len(q["ray_mask"]) == FR.SCENE_R and int(q["ray_mask"].sum()) == FR.SCENE_HIT["C"]
    pix = sc["pixel_idx"]
    vs = q["geo"].vscale
    occupied = q["occ"][pix[:, 0] // int(vs[0]), pix[:, 1] // int(vs[1])].sum(-1)
    hit = q["ray_mask"] > 0
    assert int(((occupied >= sc["opt"].SR) & hit).sum()) == 856      # rays that fill all 8 slots ...
    assert int(((occupied > sc["opt"].SR) & hit).sum()) == 844       # ... and those whose column holds more ids
    e = _bufs(sc, q)
    assert int((e["n_filled"] == sc["opt"].SR).sum()) == 856
    assert np.array_equal(e["n_filled"], np.where(q["ray_mask"] > 0, np.minimum(occupied, sc["opt"].SR), 0))


@pytest.mark.parametrize("name", "ABC")
def test_expected_buffers_invariants(scenes, name):
    sc, q = scenes[name]
    SR, K = int(sc["opt"].SR), int(sc["opt"].K)
    e = _bufs(sc, q)
    FR.check_invariants(e, FR.SCENE_R, SR, K)
    # a subset in shuffled order, plus one pixel outside the frame: each ray's rows are those of the full frame
    for sub in FR.subsets():
        pix = np.concatenate([sc["pixel_idx"][sub], [[sc["W"], 0]]]).astype(np.int32)
        qs = FR.ref_query(sc, pix)
        es = _bufs(sc, qs)
        FR.check_invariants(es, len(pix), SR, K)
        assert es["ray_hit"][-1] == 0 and es["n_filled"][-1] == 0
        assert np.array_equal(es["ray_hit"][:-1], e["ray_hit"][sub])
        assert np.array_equal(es["n_filled"][:-1], e["n_filled"][sub])
        for i in (0, len(sub) // 2, len(sub) - 1):
            a, n = es["ray_off"][i], es["n_filled"][i]
            a0 = e["ray_off"][sub[i]]
            assert np.array_equal(es["pidx"][a:a + n], e["pidx"][a0:a0 + n])
            assert np.array_equal(es["sample_p"][a:a + n], e["sample_p"][a0:a0 + n])


def test_expected_buffers_of_missing_rays_and_empty_batches(scenes):
    sc, q = scenes["A"]
    SR, K = int(sc["opt"].SR), int(sc["opt"].K)
    miss = np.nonzero(q["ray_mask"] == 0)[0][:7]
    e = _bufs(sc, FR.ref_query(sc, sc["pixel_idx"][miss]))
    FR.check_invariants(e, 7, SR, K)
    assert list(e["counts"]) == [0, 0, 0, 0, 0] and not e["ray_off"].any()
    e = _bufs(sc, FR.ref_query(sc, np.zeros((0, 2), np.int32)))
    FR.check_invariants(e, 0, SR, K)
    e = _bufs(sc, FR.ref_query(sc, pers=np.zeros((0, 3), np.float32)))
    FR.check_invariants(e, FR.SCENE_R, SR, K)
    assert not e["ray_hit"].any()


def test_z_unfilled_is_the_centre_of_depth_id_minus_one(scenes):
    import pquery_ref as PR
    _, q = scenes["A"]
    assert FR.z_unfilled(q["geo"]) == float(PR.centre(q["geo"], 0, 0, -1)[2])
    unfilled = q["slot_z"] < 0
    assert unfilled.any() and (q["sample_loc"][unfilled][:, 2] == np.float32(FR.z_unfilled(q["geo"]))).all()


def test_perspective_cases_cover_the_lists():
    assert {c[0] for c in FR.P_CASES} == set(FR.P_SR)
    for sr in FR.P_SR:   # every SR with both C, with bg and without, with both unit modes
        for key, vals in ((1, {3, 128}), (2, {True, False}), (3, {0, 1})):
            assert {c[key] for c in FR.P_CASES if c[0] == sr} == vals


@pytest.mark.parametrize("SR,C,bg,unit", FR.P_CASES)
def test_fp32_restatement_meets_bar_perspective(SR, C, bg, unit):
    b, feat, bgc, hit, zs = FR.case_inputs(SR, C, bg, unit)
    vc, nf = b["ray_vcnt"].numpy(), b["n_filled"].numpy()
    h = hit.numpy()
    assert ((h == 1) & (vc == 0)).any() and (SR == 1 or ((h == 0) & (nf > 0)).any())
    z = b["sample_p"].numpy()[:, 2]
    assert zs[0] < z.min() and z.min() < zs[1] < z.max() and zs[2] > z.max()
    params = dict(vsize_z=CR.VSIZE_Z, unit=unit, bg=bgc)
    w = CR.Worst()
    for zu in zs:
        a = FR.composite_reference_p(b, feat, hit, zu, params, torch.float32)
        r = FR.composite_reference_p(b, feat, hit, zu, params, torch.float64)
        assert torch.equal(a["ray_mask"], hit)
        for k in ("ray_color", "opacity", "is_bg"):
            assert torch.isfinite(a[k]).all()
            w.close(a[k], r[k], k, ABS.get(k, 0.0), what=f"fp32 restatement SR={SR} C={C} zu={zu:.4f}")
        # a hit ray without a valid sample, in fp32 (where 1 + 1e-10 is 1): opacity 0, colour bg, is_bg 1
        e = torch.from_numpy((h == 1) & (vc == 0))
        assert (a["opacity"][e] == 0).all() and (a["is_bg"][e] == 1).all()
        assert torch.equal(a["ray_color"][e], (bgc if bg else torch.zeros(C)).expand(int(e.sum()), C))
    # the unfilled depth matters (without the unit clamp, which maps every step past 2 vsize_z to vsize_z)
    r0, r2 = (FR.composite_reference_p(b, feat, hit, zu, params, torch.float64) for zu in (zs[0], zs[2]))
    if SR > 1 and not unit:
        assert not np.array_equal(r0["ray_dist"], r2["ray_dist"])
