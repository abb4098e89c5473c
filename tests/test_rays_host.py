"""Ray batches, the part that needs no GPU: the restatement's generator against
the Random123 known answers, its picks' ranges, and the host-side argument
checks of pnr_camera_rays / pnr_ray_batch (they run before any HIP call; the
pointers are never dereferenced)."""
import numpy as np
import pytest

import rays_ref as RR


def test_philox_known_answers():
    for ctr, key, want in RR.KNOWN:
        got = tuple(int(v) for v in RR.philox4x32_10(ctr, key))
        assert got == want, [hex(v) for v in got]
    # vectorised over the first counter word = the scalar calls
    i = np.arange(5, dtype=np.uint64)
    vec = RR.words(7, 2 ** 32 + 5, i, 0)
    for n in range(5):
        assert [int(v[n]) for v in vec] == [int(v) for v in RR.words(7, 2 ** 32 + 5, n, 0)]
    assert [int(v) for v in RR.words(7, 2 ** 32 + 5, 0, 0)] != [int(v) for v in RR.words(7, 5, 0, 0)]


def test_picks_stay_inside_the_image():
    H, W = 7, 5
    white = []
    for step in list(range(1000)) + [2 ** 32 + 5]:
        px, py = RR.picks("random", 3, step, H, W, 4)
        assert px.shape == (16,) and px.min() >= 0 and px.max() < W and py.min() >= 0 and py.max() < H
        for S in (2, 5):
            (ox, oy), w, f = RR.batch_draw(3, step, 3, H, W, S)
            assert 0 <= ox <= W - S and 0 <= oy <= H - S and 0 <= f < 3
            qx, qy = RR.picks("patch", 3, step, H, W, S)
            assert qx.min() == ox and qx.max() == ox + S - 1 and qy.min() == oy and qy.max() == oy + S - 1
            assert qx[1] == ox + 1 and qy[1] == oy and qy[S] == oy + 1     # meshgrid order: x fastest
        white.append(w)
    assert 0.4 < np.mean(white) < 0.6
    fx, fy = RR.picks("full", 3, 0, H, W)
    assert fx[:6].tolist() == [0, 1, 2, 3, 4, 0] and fy[:6].tolist() == [0, 0, 0, 0, 0, 1] and fx.shape == (35,)
    # every pixel and every frame is reachable
    px, py = RR.picks("random", 0, 0, H, W, 30)
    assert set(zip(px.tolist(), py.tolist())) == {(x, y) for x in range(W) for y in range(H)}
    assert {RR.batch_draw(0, s, 3, H, W)[2] for s in range(64)} == {0, 1, 2}


def _lib():
    from pointnerf_amd import _lib as L
    return L, L.lib(), L.c_void_p(0x1000)


def test_camera_rays_refuses_bad_arguments():
    L, lib, p = _lib()
    ok = dict(cams=p, F=1, frame=0, H=7, W=5, pixels=None, R=35, dir_norm=0, raydir=p, pixel_idx=None)
    cases = [(dict(cams=None), b"null"), (dict(raydir=None), b"null"), (dict(F=0), b"F=0"),
             (dict(frame=1), b"frame 1"), (dict(frame=-1), b"frame -1"), (dict(H=0), b"H=0"),
             (dict(H=65536, W=32769, R=65536 * 32769), b"above 2^31"),
             (dict(pixels=p, R=2 ** 31 + 1), b"R=2147483649"), (dict(R=-1), b"R=-1"),
             (dict(R=34), b"no pixel list")]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.pnr_camera_rays(a["cams"], a["F"], a["frame"], a["H"], a["W"], a["pixels"], a["R"], a["dir_norm"],
                                 a["raydir"], a["pixel_idx"], None)
        assert rc == L.PNR_EINVAL, change
        assert msg in lib.pnr_last_error(), (change, lib.pnr_last_error())


def test_ray_batch_refuses_bad_arguments():
    L, lib, p = _lib()
    names = ("images", "images_u8", "cams", "F", "H", "W", "state", "frame", "frame_dev", "mode", "S", "dir_norm",
             "bg_mode", "raydir", "pixel_idx", "gt", "campos", "camrot", "bg", "frame_id")
    ok = dict(images=p, images_u8=1, cams=p, F=3, H=7, W=5, state=p, frame=-1, frame_dev=None, mode=0, S=4,
              dir_norm=0, bg_mode=1, raydir=p, pixel_idx=p, gt=p, campos=p, camrot=p, bg=p, frame_id=p)
    cases = [(dict([(k, None)]), b"null") for k in ("images", "cams", "state", "raydir", "pixel_idx", "gt", "campos",
                                                    "camrot", "bg", "frame_id")]
    cases += [(dict(mode=3), b"unknown mode 3"), (dict(mode=-1), b"unknown mode -1"),
              (dict(bg_mode=4), b"unknown bg mode 4"), (dict(S=0), b"S=0"), (dict(mode=1, S=0), b"S=0"),
              (dict(mode=1, S=6), b"patch S=6 above min(H, W)=5"), (dict(F=0), b"F=0"), (dict(frame=3), b"frame 3"),
              (dict(W=0), b"W=0"), (dict(mode=2, H=65536, W=32769), b"above 2^31"),
              (dict(S=46341), b"above 2^31")]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.pnr_ray_batch(*(a[k] for k in names), None)
        assert rc == L.PNR_EINVAL, change
        assert msg in lib.pnr_last_error(), (change, lib.pnr_last_error())


def test_frame_set_refuses_unbuilt_modes_by_name():
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.rays import FrameSet, mode_code
    assert mode_code("no_crop") == mode_code("full_image") == mode_code("full") == 2
    assert (mode_code("random"), mode_code("patch")) == (0, 1)
    fs = FrameSet.__new__(FrameSet)     # the mode is checked before the set is looked at: no GPU needed
    for name in ("random2", "proportional_random"):
        with pytest.raises(PnrError, match=name):
            fs.sample(4, mode=name)
    with pytest.raises(PnrError, match="unknown random_sample 'stripes'"):
        fs.sample(4, mode="stripes")
