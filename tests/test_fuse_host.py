"""Depth-map fusion, the part that needs no GPU: the fp64 restatement
(fuse_ref.py) on cases worked out by hand, the scene the GPU test assumes, and
the host-side argument checks of pnr_depth_fuse_scratch_bytes / pnr_depth_fuse
/ pnr_depth_points (they run before any HIP call; the pointers are never
dereferenced)."""
import numpy as np
import pytest

import fuse_ref as FR
from pointnerf_amd import fuse_depth_maps  # noqa: F401  (the feature under test)

CASES = FR.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_on_hand_built_cases(name):
    c = CASES[name]
    r = FR.fuse(c["depths"], c["cams"], **c["kwargs"])
    for key in ("count", "visible", "keep"):
        assert np.array_equal(r[key], c[key]), key
    if "depth_avg" in c:    # every operation of these cases is exact
        assert np.array_equal(r["depth_avg"], np.asarray(c["depth_avg"], np.float32).astype(np.float64))
    assert r["src_pixel"].tolist() == np.nonzero(c["keep"].reshape(-1))[0].tolist()
    assert np.array_equal(r["count_out"], c["count"].reshape(-1)[r["src_pixel"]])


def test_restatement_pair_quantities():
    """plane: view 0's pixel (i, j) lands on (i - 0.5, j + 0.5) of view 1 and
    comes back on itself at the same depth; scaled: 2 % off in depth; behind: a
    point behind the source camera has no sample."""
    r = FR.fuse(CASES["plane"]["depths"], CASES["plane"]["cams"], geo_cnsst_num=1)
    jj, ii = np.mgrid[:FR.HAND_H, :FR.HAND_W]
    assert np.array_equal(r["u"][0, 1], ii - 0.5) and np.array_equal(r["v"][0, 1], jj + 0.5)
    assert np.array_equal(r["vis"][0, 1], ii >= 1) and r["taps_ok"][0, 1].all()
    assert not r["dist"][0, 1][:, 1:].any() and not r["rel"][0, 1][:, 1:].any()
    assert np.isnan(r["dist"][0, 1][:, 0]).all() and np.isnan(r["u"][0, 0]).all()
    r = FR.fuse(CASES["scaled"]["depths"], CASES["scaled"]["cams"])
    assert np.allclose(r["rel"][0, 1][:, 1:], 0.02, rtol=0, atol=1e-7)            # 4.08 against 4
    assert np.allclose(r["rel"][1, 0][:, :-1], 0.08 / 4.08, rtol=0, atol=1e-7)    # 4 against 4.08
    r = FR.fuse(CASES["behind"]["depths"], CASES["behind"]["cams"])
    assert not r["vis"][0, 1].any() and np.isnan(r["dist"][0, 1]).all()
    assert r["vis"][1, 0].all() and np.array_equal(r["cz2"][1, 0], np.full((FR.HAND_H, FR.HAND_W), -1.0))
    r = FR.fuse(CASES["straddle"]["depths"], CASES["straddle"]["cams"])
    assert np.array_equal(~r["taps_ok"][0, 1], (ii >= 3) & (ii <= 4) & (jj >= 1) & (jj <= 2))


def test_restatement_keep_rule_options():
    c = CASES["plane"]
    conf = np.full((2, FR.HAND_H, FR.HAND_W), 0.5, np.float32)
    conf[0, 3, 3], conf[0, 3, 4] = 0.25, np.float32(0.3)
    mask = np.ones((2, FR.HAND_H, FR.HAND_W), np.uint8)
    mask[1, 0, 0] = 0
    base = FR.fuse(c["depths"], c["cams"], geo_cnsst_num=1)
    r = FR.fuse(c["depths"], c["cams"], conf=conf, mask=mask, conf_thresh=0.3, geo_cnsst_num=1)
    gone = base["keep"] & ~r["keep"]
    assert sorted(zip(*np.nonzero(gone))) == [(0, 3, 3), (0, 3, 4), (1, 0, 0)]    # conf > thresh is strict
    assert np.array_equal(r["conf"], conf.reshape(-1)[r["src_pixel"]])
    # the plane z = 0 spans x = i - 3.5 in view 0: the closed box keeps x in [-0.5, 1.5], pixels 3 .. 5
    r = FR.fuse(c["depths"], c["cams"], ranges=(-0.5, -10, -1, 1.5, 10, 1), geo_cnsst_num=1)
    assert np.array_equal(r["keep"][0], base["keep"][0] & (np.mgrid[:FR.HAND_H, :FR.HAND_W][1] >= 3) &
                          (np.mgrid[:FR.HAND_H, :FR.HAND_W][1] <= 5))
    assert np.array_equal(FR.fuse(c["depths"], c["cams"], ranges=(-100, 0, 0, 0, 0, 0), geo_cnsst_num=1)["keep"],
                          base["keep"])
    # geo_cnsst_num above the one match there is: nothing left; with reassign_conf count 1 at geo 1 -> k = 1
    assert not FR.fuse(c["depths"], c["cams"], geo_cnsst_num=2)["keep"].any()
    r = FR.fuse(c["depths"], c["cams"], geo_cnsst_num=1, reassign_conf=True)
    assert np.allclose(r["conf"], 1 - 1 / 1.14869, rtol=0, atol=1e-7)
    r = FR.fuse(c["depths"], c["cams"], geo_cnsst_num=0, reassign_conf=True)      # k = clamp(count + 1, 1, 10)
    assert np.allclose(r["conf"], 1 - 1 / 1.14869 ** (r["count_out"] + 1), rtol=0, atol=1e-7)


def test_main_scene_is_what_the_gpu_test_assumes():
    s = FR.scene()
    r = FR.fuse(s["depths"], s["cams"])
    assert int(r["valid"].sum()) == 15692 and int(r["valid"].sum()) * 7 == 109844
    assert int(r["match"].sum()) == 27064
    assert np.bincount(r["count"][r["valid"]]).tolist() == [3133, 4453, 3830, 2483, 1463, 330]
    assert len(r["src_pixel"]) == 2483 + 1463 + 330
    assert round(len(r["src_pixel"]) / 15692, 2) == 0.27
    # both outcomes of every test occur
    assert (r["vis"] & ~r["taps_ok"]).any() and (r["visible"][r["valid"]] < 7).any()
    with np.errstate(invalid="ignore"):
        assert (r["dist"] >= 1).any() and (r["rel"] >= 0.01).any() and ((r["dist"] < 1) & (r["rel"] >= 0.01)).any()
    band = FR.banded(r, s["W"], s["H"]) & r["valid"]
    assert int(band.sum()) == 42
    # the scaled view 3 agrees with few (only where the 2 % slide along a grazing ray stays inside both thresholds)
    per_view = r["match"].sum((1, 2, 3))
    assert per_view.tolist() == [3951, 3877, 3352, 719, 3406, 3799, 4002, 3958]


@pytest.mark.parametrize("shape", [{}, dict(H=47, W=61), dict(F=65, H=12, W=16, focal=25.0)],
                         ids=["main", "61x47", "F65"])
def test_fp32_twin_differs_from_fp64_only_inside_the_bands(shape):
    """The same restatement in fp32 decides like fp64 outside the banded pixels,
    its error on the pairs within ten bands of a threshold is at least 5 x
    inside the bands, and banded pixels stay below 1 % of the valid ones."""
    s = FR.scene(**shape)
    r, t = FR.fuse(s["depths"], s["cams"]), FR.fuse(s["depths"], s["cams"], dtype=np.float32)
    band = FR.banded(r, s["W"], s["H"])
    assert (band & r["valid"]).sum() <= 0.01 * r["valid"].sum()
    for key in ("count", "visible", "keep"):
        assert np.array_equal(r[key][~band], t[key][~band]), key
    du, ddist, drel = FR.twin_errors(r, t)
    print(f"twin: max |du| {du:.3e} px, |ddist| {ddist:.3e} px, |drel| {drel:.3e}")
    assert du * 5 <= FR.EDGE_BAND and ddist * 5 <= FR.PIX_BAND and drel * 5 <= FR.REL_BAND


# ------------------------------------------------------------ argument checks
def _lib():
    from pointnerf_amd import _lib as L
    return L, L.lib(), L.c_void_p(0x1000)


def _refused(L, lib, fn, names, ok, cases):
    for change, msg in cases:
        a = dict(ok, **change)
        rc = fn(*(a[k] for k in names), None)
        assert rc == L.PNR_EINVAL, change
        assert msg in lib.pnr_last_error(), (change, lib.pnr_last_error())


def _params(L, **kw):
    from pointnerf_amd.fuse import fuse_params
    return L.ctypes.byref(fuse_params(**kw))


def test_depth_fuse_refuses_bad_arguments():
    L, lib, p = _lib()
    nb = L.c_size_t(0)
    assert lib.pnr_depth_fuse_scratch_bytes(3, 5, 37, L.ctypes.byref(nb)) == L.PNR_OK and nb.value >= 556 * 4
    assert lib.pnr_depth_fuse_scratch_bytes(3, 5, 37, None) == L.PNR_EINVAL
    assert lib.pnr_depth_fuse_scratch_bytes(0, 5, 37, L.ctypes.byref(nb)) == L.PNR_EINVAL
    assert lib.pnr_depth_fuse_scratch_bytes(128, 4096, 4096, L.ctypes.byref(nb)) == L.PNR_EINVAL
    assert b"not below 2^31" in lib.pnr_last_error()
    names = ("depths", "conf", "mask", "cams", "F", "H", "W", "params", "depth_avg", "count", "visible", "keep",
             "src", "cap", "count_dev", "scratch", "scratch_bytes")
    ok = dict(depths=p, conf=None, mask=None, cams=p, F=3, H=5, W=37, params=_params(L), depth_avg=p, count=p,
              visible=p, keep=p, src=p, cap=555, count_dev=p, scratch=p, scratch_bytes=nb.value)
    cases = [(dict([(k, None)]), b"null") for k in ("depths", "cams", "params", "depth_avg", "count", "visible",
                                                    "keep", "src", "count_dev", "scratch")]
    cases += [(dict(F=0), b"F=0"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"),
              (dict(F=128, H=4096, W=4096), b"F*H*W=2147483648 not below 2^31"),
              (dict(cap=554), b"outputs hold 554 pixels, 555 may survive"),
              (dict(scratch_bytes=nb.value - 1), b"scratch too small"),
              (dict(params=_params(L, pix_thresh=0.0)), b"pix_thresh=0"),
              (dict(params=_params(L, rel_thresh=-0.01)), b"rel_thresh=-0.01"),
              (dict(params=_params(L, rel_thresh=float("nan"))), b"rel_thresh=nan"),
              (dict(params=_params(L, geo_cnsst_num=-1)), b"geo_cnsst_num=-1")]
    _refused(L, lib, lib.pnr_depth_fuse, names, ok, cases)


def test_depth_points_refuses_bad_arguments():
    L, lib, p = _lib()
    names = ("src", "M", "depth_avg", "count_map", "conf", "cams", "F", "H", "W", "params", "xyz", "conf_out",
             "src_pixel", "count_out", "cap")
    ok = dict(src=p, M=10, depth_avg=p, count_map=p, conf=None, cams=p, F=3, H=5, W=37, params=_params(L), xyz=p,
              conf_out=p, src_pixel=p, count_out=p, cap=10)
    cases = [(dict([(k, None)]), b"null") for k in ("src", "depth_avg", "count_map", "cams", "params", "xyz",
                                                    "conf_out", "src_pixel", "count_out")]
    cases += [(dict(M=-1), b"M=-1"), (dict(M=556, cap=556), b"M=556 outside [0, F*H*W=555]"), (dict(F=0), b"F=0"),
              (dict(H=0), b"H=0"), (dict(W=0), b"W=0"), (dict(cap=9), b"outputs hold 9 points, M=10"),
              (dict(params=_params(L, pix_thresh=-1.0)), b"pix_thresh=-1")]
    _refused(L, lib, lib.pnr_depth_points, names, ok, cases)
    # nothing to do is not an error, and launches nothing
    a = dict(ok, M=0, cap=0, src=None, xyz=None, conf_out=None, src_pixel=None, count_out=None)
    assert lib.pnr_depth_points(*(a[k] for k in names), None) == L.PNR_OK


def test_fuse_depth_maps_refuses_what_it_does_not_take():
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.fuse import fuse_params
    with pytest.raises(PnrError, match="FrameSet"):
        fuse_depth_maps(np.ones((2, 4, 4), np.float32), frames=None)
    with pytest.raises(PnrError, match="6 values"):
        fuse_params(ranges=(0, 0, 0, 1, 1))
    assert fuse_params().ranges[0] <= -99 and fuse_params().geo_cnsst_num == 3
