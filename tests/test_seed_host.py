"""Point seeding, the part that needs no GPU: the fp64 restatement
(seed_ref.py) on cases worked out by hand, and the host-side argument checks
of pnr_alpha_bits / pnr_seed_mask / pnr_seed_view (they run before any HIP
call; the pointers are never dereferenced)."""
import numpy as np
import pytest

import seed_ref as SR
from pointnerf_amd import seed_points  # noqa: F401  (the feature under test)

CASES = SR.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_on_hand_built_cases(name):
    c = CASES[name]
    r = SR.seed(c["xyz"], c["cams"], c["images"], c["alphas"], **c["kwargs"])
    assert r["keep"].tolist() == c["keep"]
    assert r["src_idx"].tolist() == [i for i, k in enumerate(c["keep"]) if k]
    for key in ("cam_ind", "in_view"):
        if key in c:
            assert r[key].tolist() == c[key]
    if "color" in c:
        assert np.array_equal(r["color"], np.asarray(c["color"]))   # a pixel centre: weights 1 and 0, exact


def test_restatement_direction_and_border_taps():
    c = CASES["on_ray"]
    r = SR.seed(c["xyz"], c["cams"], c["images"], c["alphas"])
    d = np.array([0.75, -0.75, 2.0])
    n = np.sqrt(d @ d)
    assert np.allclose(r["dirs"][0], d / (n + 1e-6), rtol=0, atol=1e-12)
    # the image corner, (u, v) = (0.25, 0.25): every tap clamps to texel (0, 0)
    p = np.array([[(0.25 - 4) / 4 * 2, (0.25 - 3) / 4 * 2, -1.0]], np.float32)
    r = SR.seed(p, c["cams"], c["images"], None)
    assert r["in_view"].tolist() == [True]
    assert np.allclose(r["color"][0], c["images"][0, 0, 0] / 255.0, rtol=0, atol=1e-12)
    # half-way between texels (2, 2) and (3, 2): (u, v) = (3.0, 2.5)
    p = np.array([[(3.0 - 4) / 4 * 2, (2.5 - 3) / 4 * 2, -1.0]], np.float32)
    r = SR.seed(p, c["cams"], c["images"], None)
    want = (c["images"][0, 2, 2].astype(np.float64) + c["images"][0, 2, 3]) / 2 / 255.0
    assert np.allclose(r["color"][0], want, rtol=0, atol=1e-12)
    # out of view: colour 0, in_view 0, the direction still there
    p = np.array([[-3.0, 0, -1.0]], np.float32)
    r = SR.seed(p, c["cams"], c["images"], None)
    assert r["in_view"].tolist() == [False] and not r["color"].any() and abs(np.linalg.norm(r["dirs"][0]) - 1) < 1e-5


def test_main_scene_is_what_the_gpu_test_assumes():
    s = SR.scene()
    r = SR.seed(s["xyz"], s["cams"], s["images"], s["alphas"])
    assert len(r["src_idx"]) == 4972
    assert r["in_view"].all() and set(r["cam_ind"].tolist()) == set(range(12))
    c = SR.cam_coords(r["xyz"], s["cams"])
    u, v = SR.pixel_pos(c, s["cams"])
    assert SR.inside(u, v, c[..., 2], s["H"], s["W"]).all()      # every survivor, every camera
    # inall_img never comes into play: a point outside some image is carved by another view anyway
    assert np.array_equal(SR.mask(s["xyz"], s["cams"], s["H"], s["W"], s["alphas"], inall_img=0), r["keep"])


def _lib():
    from pointnerf_amd import _lib as L
    return L, L.lib(), L.c_void_p(0x1000)


def _refused(L, lib, fn, names, ok, cases):
    for change, msg in cases:
        a = dict(ok, **change)
        rc = fn(*(a[k] for k in names), None)
        assert rc == L.PNR_EINVAL, change
        assert msg in lib.pnr_last_error(), (change, lib.pnr_last_error())


def test_alpha_bits_refuses_bad_arguments():
    L, lib, p = _lib()
    names = ("alphas", "u8", "F", "H", "W", "bits", "pitch", "words")
    ok = dict(alphas=p, u8=0, F=3, H=5, W=37, bits=p, pitch=2, words=30)
    cases = [(dict(alphas=None), b"null"), (dict(bits=None), b"null"), (dict(F=0), b"F=0"), (dict(H=0), b"H=0"),
             (dict(W=0, pitch=0), b"W=0"), (dict(pitch=1), b"pitch of 1 words, W=37 needs 2"),
             (dict(pitch=3), b"pitch of 3 words"), (dict(words=29), b"bits holds 29 words, 30 needed")]
    _refused(L, lib, lib.pnr_alpha_bits, names, ok, cases)


def test_seed_mask_refuses_bad_arguments():
    L, lib, p = _lib()
    nb = L.c_size_t(0)
    assert lib.pnr_seed_scratch_bytes(1000, L.ctypes.byref(nb)) == L.PNR_OK and nb.value >= 1001 * 4
    assert lib.pnr_seed_scratch_bytes(1000, None) == L.PNR_EINVAL
    assert lib.pnr_seed_scratch_bytes(-1, L.ctypes.byref(nb)) == L.PNR_EINVAL
    names = ("xyz", "N", "cams", "F", "H", "W", "bits", "pitch", "ranges", "near_far", "inall", "keep", "src", "cap",
             "count", "scratch", "scratch_bytes")
    ok = dict(xyz=p, N=1000, cams=p, F=3, H=5, W=37, bits=p, pitch=2, ranges=None, near_far=None, inall=1, keep=p,
              src=p, cap=1000, count=p, scratch=p, scratch_bytes=nb.value)
    cases = [(dict([(k, None)]), b"null") for k in ("xyz", "cams", "keep", "src", "count", "scratch")]
    cases += [(dict(N=0), b"N=0"), (dict(N=2 ** 31), b"N=2147483648"), (dict(F=0), b"F=0"), (dict(H=0), b"H=0"),
              (dict(W=0), b"W=0"), (dict(pitch=1), b"pitch of 1 words, W=37 needs 2"),
              (dict(cap=999), b"outputs hold 999 points, 1000 may survive"),
              (dict(scratch_bytes=nb.value - 1), b"scratch too small")]
    _refused(L, lib, lib.pnr_seed_mask, names, ok, cases)


def test_seed_view_refuses_bad_arguments():
    L, lib, p = _lib()
    names = ("xyz", "M", "images", "u8", "cams", "F", "H", "W", "cam_ind", "dirs", "color", "in_view", "cap")
    ok = dict(xyz=p, M=10, images=p, u8=1, cams=p, F=3, H=5, W=37, cam_ind=p, dirs=p, color=p, in_view=p, cap=10)
    cases = [(dict([(k, None)]), b"null") for k in ("xyz", "images", "cams", "cam_ind", "dirs", "color", "in_view")]
    cases += [(dict(M=-1), b"M=-1"), (dict(F=0), b"F=0"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"),
              (dict(H=65536, W=32769), b"above 2^31"), (dict(cap=9), b"outputs hold 9 points, M=10")]
    _refused(L, lib, lib.pnr_seed_view, names, ok, cases)
    # nothing to do is not an error, and launches nothing
    a = dict(ok, M=0, cap=0, xyz=None, cam_ind=None, dirs=None, color=None, in_view=None)
    assert lib.pnr_seed_view(*(a[k] for k in names), None) == L.PNR_OK


def test_seed_points_refuses_what_it_does_not_take():
    from pointnerf_amd._lib import PnrError
    with pytest.raises(PnrError, match="FrameSet"):
        seed_points(np.zeros((4, 3), np.float32), frames=None)
