"""seed_points (pnr_alpha_bits / pnr_seed_mask / pnr_seed_view) against the
fp64 restatement tests/seed_ref.py.

Rule: the survivor set and each survivor's view are compared exactly, except
for the points the fp64 reference itself puts within reach of fp32 rounding: a
pixel coordinate within 1e-4 px of an integer in some view (the hull vote, and
in_view, may fall either way) or best two view scores within 1e-5 (either of
the two views may win).  Those are at most 1 % of the main scene (0.63 % in the
reference alone) and must still give one of the two admissible answers.  dirs
within 2e-6 absolute (a few ulp of a unit vector), color within 1e-4 absolute
(the sample is 1-Lipschitz per axis in the pixel coordinate for a [0,1] image,
|du| is a few ulp of 64, two axes: about 6e-5), both against the reference
evaluated in the view the device chose."""
import numpy as np
import pytest
import torch

import seed_ref as SR
from pointnerf_amd import seed_points

pytestmark = pytest.mark.gpu

PIX_BAND, TIE_BAND = 1e-4, 1e-5
DIR_TOL, COLOR_TOL = 2e-6, 1e-4
_SCENES = {}


def _scene(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _SCENES:
        _SCENES[key] = SR.scene(**kw)
    return _SCENES[key]


def _frames(s, cuda, images=None):
    from pointnerf_amd.rays import FrameSet
    return FrameSet(s["images"] if images is None else images, (s["campos"], s["camrot"]), s["K"], 2.0, 6.0,
                    device=cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _check_shapes(out, n_in):
    m = out["xyz"].shape[0]
    want = dict(xyz=((m, 3), torch.float32), embedding=((1, m, 32), torch.float32), color=((1, m, 3), torch.float32),
                dirs=((1, m, 3), torch.float32), conf=((1, m, 1), torch.float32), cam_ind=((m,), torch.int32),
                src_idx=((m,), torch.int64), in_view=((m,), torch.bool))
    assert set(out) == set(want)
    for k, (shape, dtype) in want.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].is_cuda, k
    src = _np(out["src_idx"])
    assert m == 0 or (src.min() >= 0 and src.max() < n_in)
    return m


def _compare(out, s, alphas=None, images=None, max_excluded=None, **kw):
    """Everything seed_points returns (vox_res = 0) against the restatement."""
    xyz, cams, H, W = s["xyz"], s["cams"], s["H"], s["W"]
    images = s["images"] if images is None else images
    n = len(xyz)
    _check_shapes(out, n)
    keep_ref = SR.mask(xyz, cams, H, W, alphas, **kw)
    c = SR.cam_coords(xyz, cams)
    u, v = SR.pixel_pos(c, cams)
    with np.errstate(invalid="ignore"):
        near_int = (np.abs(u - np.round(u)) < PIX_BAND) | (np.abs(v - np.round(v)) < PIX_BAND)
    ex_pix = near_int.any(1)
    scores = SR.view_scores(xyz, cams, H, W)
    order = np.argsort(scores, 1, kind="stable")
    rows = np.arange(n)
    ex_tie = (scores[rows, order[:, min(1, scores.shape[1] - 1)]] - scores[rows, order[:, 0]] < TIE_BAND) \
        if scores.shape[1] > 1 else np.zeros(n, bool)
    share = float((ex_pix | ex_tie).mean())
    print(f"N {n} kept {int(keep_ref.sum())} excluded: pixel {int(ex_pix.sum())} tie {int(ex_tie.sum())} "
          f"share {share:.4f}")
    if max_excluded is not None:
        assert share <= max_excluded

    src = _np(out["src_idx"])
    assert np.all(np.diff(src) > 0), "src_idx not strictly increasing"
    assert np.array_equal(_np(out["xyz"]).view(np.uint32), xyz[src].view(np.uint32)), "xyz != input[src_idx] bitwise"
    keep = np.zeros(n, bool)
    keep[src] = True
    wrong = (keep != keep_ref) & ~ex_pix
    print(f"survivors {len(src)}; differ from fp64 {int((keep != keep_ref).sum())}, outside the band {int(wrong.sum())}")
    assert not wrong.any(), np.nonzero(wrong)[0][:10]

    cam = _np(out["cam_ind"]).astype(np.int64)
    best, second = order[src, 0], order[src, min(1, scores.shape[1] - 1)]
    bad = (cam != best) & ~(ex_tie[src] & (cam == second))
    print(f"cam_ind differ from fp64 {int((cam != best).sum())}, inadmissible {int(bad.sum())}")
    assert not bad.any(), src[bad][:10]

    _, dirs, color, seen = SR.view(xyz[src], cams, images, H, W, cam_ind=cam)
    got_seen = _np(out["in_view"])
    bad = (got_seen != seen) & ~near_int[src, cam]
    assert not bad.any(), src[bad][:10]
    d_err = np.abs(_np(out["dirs"])[0] - dirs).max(initial=0.0)
    both = got_seen & seen
    c_err = np.abs(_np(out["color"])[0] - color)[both].max(initial=0.0)
    print(f"max |dirs - ref| {d_err:.3e} (tol {DIR_TOL}), max |color - ref| {c_err:.3e} (tol {COLOR_TOL}), "
          f"in view {int(both.sum())}")
    assert d_err <= DIR_TOL
    assert c_err <= COLOR_TOL
    assert not _np(out["color"])[0][~got_seen].any(), "a point out of view has a colour"
    assert np.all(_np(out["conf"]) == 1.0)
    return src


# ------------------------------------------------------------------ main scene
def test_main_scene_matches_fp64(cuda):
    s = _scene()
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=s["alphas"])
    src = _compare(out, s, alphas=s["alphas"], max_excluded=0.01)
    assert abs(len(src) - 4972) <= 92
    assert set(_np(out["cam_ind"]).tolist()) == set(range(12))
    assert _np(out["in_view"]).all()


@pytest.mark.parametrize("opts", [dict(ranges=(-0.5, -0.6, -0.7, 0.4, 0.55, 0.65)), dict(near_far=(3.25, 3.4)),
                                  dict(inall_img=0), dict(inall_img=1)],
                         ids=["ranges", "near_far", "inall0", "inall1"])
def test_main_scene_options(cuda, opts):
    s = _scene()
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=s["alphas"], **opts)
    src = _compare(out, s, alphas=s["alphas"], **opts)
    assert 0 < len(src) <= 4972 + 92


def test_main_scene_float_images_and_uint8_alphas(cuda):
    s = _scene(float_images=True)
    assert s["images"].dtype == np.float32
    al = (s["alphas"] * 255).astype(np.uint8)
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=torch.from_numpy(al))
    _compare(out, s, alphas=al)


def test_no_alphas_keeps_everything(cuda):
    s = _scene()
    out = seed_points(s["xyz"], _frames(s, cuda))
    src = _compare(out, s)
    assert len(src) == len(s["xyz"])


# ------------------------------------------------------------- breaking shapes
def _small(F, N=1000, **kw):
    return _scene(N=N, F=F, H=8, W=8, focal=7.5, radius=2.5, **kw)


@pytest.mark.parametrize("F", [1, 64, 65], ids=["F1", "tile", "tile+1"])
def test_camera_tile_boundaries(cuda, F):
    from pointnerf_amd.seed import CAM_TILE
    assert CAM_TILE == 64
    s = _small(F)
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=s["alphas"])
    src = _compare(out, s, alphas=s["alphas"])
    assert len(src) > 50
    if F > 1:
        assert int(out["cam_ind"].max()) > F // 2        # the views past the first half win points too


def _noise_alphas(s, seed=3):
    return (np.random.default_rng(seed).random((s["F"], s["H"], s["W"]), dtype=np.float32) * 0.2).astype(np.float32)


@pytest.mark.parametrize("inall", [0, 1])
def test_row_padding_and_border_clamp(cuda, inall):
    """W = 37, H = 5: two words per row, the second mostly padding; noise masks,
    and most points project above or below the strip, so inall_img decides."""
    s = _scene(N=2000, F=3, H=5, W=37, focal=20.0)
    al = _noise_alphas(s)
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=al, inall_img=inall)
    src = _compare(out, s, alphas=al, inall_img=inall)
    assert 0 < len(src) < 2000
    assert 0 < int(out["in_view"].sum()) < len(src)      # some survivors' nearest view does not see them


@pytest.mark.parametrize("W,H,u8", [(37, 5, False), (64, 3, True), (70, 4, False), (129, 2, True)])
def test_alpha_bit_planes(cuda, W, H, u8):
    from pointnerf_amd.rays import FrameSet
    from pointnerf_amd.seed import alpha_bits
    F = 3
    rng = np.random.default_rng(W)
    al = (rng.random((F, H, W)) * 0.2).astype(np.float32)
    al.flat[:4] = [0.1, np.nextafter(np.float32(0.1), np.float32(1)), 0.0, 1.0]   # > 0.1 is strict
    if u8:
        al = rng.integers(0, 52, (F, H, W)).astype(np.uint8)                    # 25 / 255 < 0.1 < 26 / 255
    cam = SR.ring_cameras(F)
    fs = FrameSet(np.zeros((F, H, W, 3), np.uint8), cam, SR.RR.focal_K(10.0, H, W), 2.0, 6.0, device=cuda)
    bits = _np(alpha_bits(al, fs))
    pitch = (W + 31) // 32
    assert bits.shape == (F, H, pitch)
    on = np.zeros((F, H, pitch * 32), bool)
    on[..., :W] = SR.alpha_on(al)
    want = np.packbits(on, axis=-1, bitorder="little").view(np.uint32).reshape(F, H, pitch)
    assert np.array_equal(bits.view(np.uint32), want)
    assert 0.2 < on[..., :W].mean() < 0.8


def test_one_point(cuda):
    s = _small(3, N=1)
    s = dict(s, xyz=np.array([[0.1, 0.2, -0.15]], np.float32))
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=s["alphas"])
    assert _compare(out, s, alphas=s["alphas"]).tolist() == [0]


def test_every_point_carved(cuda):
    s = _small(3)
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=np.zeros_like(s["alphas"]))
    assert _check_shapes(out, len(s["xyz"])) == 0
    out = seed_points(s["xyz"], _frames(s, cuda), alphas=np.zeros_like(s["alphas"]), vox_res=8)
    assert _check_shapes(out, len(s["xyz"])) == 0


def test_voxel_downsample_composes_with_the_mask(cuda):
    from pointnerf_amd import construct_vox_points_closest
    s = _scene()
    fs = _frames(s, cuda)
    full = seed_points(s["xyz"], fs, alphas=s["alphas"])
    out = seed_points(s["xyz"], fs, alphas=s["alphas"], vox_res=16)
    m = _check_shapes(out, len(s["xyz"]))
    _, _, min_idx = construct_vox_points_closest(full["xyz"], 16)
    assert 100 < m == min_idx.numel() < full["xyz"].shape[0]
    assert torch.equal(out["src_idx"], full["src_idx"][min_idx])
    assert torch.equal(out["xyz"], torch.from_numpy(s["xyz"]).to(cuda)[out["src_idx"]])
    # the per-point outputs are those of the same points without the voxel stage
    for k in ("cam_ind", "in_view"):
        assert torch.equal(out[k], full[k][min_idx]), k
    for k in ("color", "dirs"):
        assert torch.equal(out[k], full[k][:, min_idx]), k


def test_conf_and_embedding_options(cuda):
    s = _small(3)
    fs = _frames(s, cuda)
    a = seed_points(s["xyz"], fs, alphas=s["alphas"], default_conf=0.5, seed=4)
    b = seed_points(s["xyz"], fs, alphas=s["alphas"], default_conf=1.5, seed=4)
    c = seed_points(s["xyz"], fs, alphas=s["alphas"], seed=5)
    z = seed_points(s["xyz"], fs, alphas=s["alphas"], embedding="zeros")
    assert torch.all(a["conf"] == 0.5) and torch.all(b["conf"] == 1.0) and torch.all(c["conf"] == 1.0)
    assert torch.equal(a["embedding"], b["embedding"]) and not torch.equal(a["embedding"], c["embedding"])
    assert 0.8 < float(a["embedding"].std()) < 1.2 and not z["embedding"].any()


# ------------------------------------------------------------ hand-built cases
@pytest.mark.parametrize("name", sorted(SR.hand_cases()))
def test_hand_built_cases(cuda, name):
    from pointnerf_amd.rays import FrameSet
    c = SR.hand_cases()[name]
    fs = FrameSet(c["images"], (c["campos"], c["camrot"]), SR.HAND_K, 2.0, 6.0, device=cuda)
    out = seed_points(c["xyz"], fs, alphas=c["alphas"], **c["kwargs"])
    assert _np(out["src_idx"]).tolist() == [i for i, k in enumerate(c["keep"]) if k]
    for key in ("cam_ind", "in_view"):
        if key in c:
            assert _np(out[key]).tolist() == c[key]
    if "color" in c:    # a pixel centre, every operation exact: that pixel's value / 255, correctly rounded
        want = c["images"][0, 1, 5].astype(np.float32) / np.float32(255)
        assert np.array_equal(_np(out["color"])[0, 0], want)


def test_point_on_a_camera_ray_gets_that_pixels_colour(cuda):
    """Points along the rays camera_rays gives for a frame's pixels get those
    pixels' ground-truth colours (to the colour tolerance: the points are
    rounded to fp32)."""
    from pointnerf_amd.rays import FrameSet
    s = _scene()
    one = FrameSet(s["images"][:1], (s["campos"][:1], s["camrot"][:1]), s["K"], 2.0, 6.0, device=cuda)
    item = one.frame(0)
    pts = item["campos"] + 2.5 * item["raydir"][0]
    out = seed_points(pts, one)
    assert out["xyz"].shape[0] == s["H"] * s["W"] and bool(out["in_view"].all())
    err = float((out["color"][0] - item["gt_image"][0]).abs().max())
    print(f"max |color - gt| {err:.3e}")
    assert err <= COLOR_TOL


# ------------------------------------------------------------------ round trip
def test_seeded_points_render(cuda):
    from formula import formula_params
    from pointnerf_amd import synthetic as S
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.rays import FrameSet
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    opt = lego_opt()
    H = W = 24
    cams = [S.camera(30.0 + 90.0 * f, -30.0, 4.0) for f in range(4)]
    images = np.random.default_rng(2).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    bg = torch.rand(128, generator=torch.Generator().manual_seed(1)).to(cuda)
    fs = FrameSet(images, (np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])),
                  SR.RR.focal_K(S.lego_focal(800) * H / 800.0, H, W), 2.0, 6.0, bg_color=bg, device=cuda)
    out = seed_points(S.lego_like_points(8000, seed=0), fs)
    pts = NeuralPoints(opt, cuda, **{k: out[k] for k in ("xyz", "embedding", "color", "dirs", "conf")})
    agg = PointAggregator(opt).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in formula_params(salt=0.35).items()})
    model = NeuralPointsRayMarching(opt, pts, agg.eval())
    item = fs.frame(1)
    color, opacity, is_bg, ray_mask = model.render_rays(item["campos"], item["camrotc2w"], item["raydir"][0], 2.0, 6.0,
                                                        item["bg_color"].reshape(-1))
    assert int(ray_mask.sum()) > 20
    assert torch.isfinite(color).all() and torch.isfinite(opacity).all()
