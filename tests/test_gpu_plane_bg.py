"""PlaneBackground (pnr_plane_fg_masks / pnr_plane_bg) against the fp64
restatement tests/plane_bg_ref.py.

Rule: the discrete decisions (which rays get a colour, which mask pixels are
set) are compared exactly, except for the rays and points the fp64 reference
itself puts within reach of fp32 rounding: a projected coordinate within 1e-3
px of an integer (the 0 / W-1 / H-1 bounds are integers) in some view,
|dot - 1e-3| < 1e-6, a sampled channel within 1e-4 of a fit bound, or a mask
pixel that such a point may or may not set.  Those rays must still give one of
the admissible answers (every open view in or out, to 1e-4) and are at most 2 %
of each scene's rays (asserted on the reference alone in
tests/test_plane_bg_host.py).  For the remaining rays the bar on bg is 4x the
fp32 twin's own error plus one ulp of 1.0 (the rule of DESIGN.md 19).  Every
(kernel error) / (twin error) ratio is printed as a RATIO line; the run on one
MI355X is in profiles/plane_bg_ratios.txt.

The hand-built corner case is outside that accounting: all its arithmetic is
exact in fp32, so it is compared bit for bit."""
import numpy as np
import pytest
import torch

import plane_bg_ref as PR
from pointnerf_amd import _lib as L

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _np(t):
    return t.detach().cpu().numpy()


def _frames(sc, cuda):
    from pointnerf_amd.rays import FrameSet
    return FrameSet(sc["images"], (sc["campos_f"], sc["camrot_f"]), sc["K"], 2.0, 6.0, device=cuda)


def _bg(sc, cuda, **kw):
    from pointnerf_amd import PlaneBackground
    if not kw:
        kw = dict(points_xyz=torch.from_numpy(sc["xyz"]))
    return PlaneBackground(_frames(sc, cuda), sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], **kw)


def _rays(bg, sc, cuda):
    """bg_ray [R,3] of the scene's batch, computed twice: bitwise repeatable."""
    campos = torch.from_numpy(sc["campos"]).to(cuda)[None]
    raydir = torch.from_numpy(sc["raydir"]).to(cuda)[None]
    a, b = bg.rays(campos, raydir), bg.rays(campos, raydir)
    assert a.shape == (1, len(sc["raydir"]), 3) and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b), "pnr_plane_bg is not repeatable"
    return _np(a)[0]


# ------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("name", list(PR.SCENES))
def test_scene_matches_fp64(cuda, name):
    sc = PR.named_scene(name)
    assert sc["images"].dtype == (np.float32 if "float" in name else np.uint8)
    assert (sc["H"], sc["W"]) == (29, 37) and (sc["h"], sc["w"]) != (sc["H"], sc["W"])
    bg = _bg(sc, cuda)
    fg = _np(bg.fg_masks).copy()
    assert fg.dtype == np.uint8 and set(np.unique(fg)) <= {0, 1}
    assert np.array_equal(_np(bg.refresh_fg(torch.from_numpy(sc["xyz"]))), fg), "pnr_plane_fg_masks is not repeatable"
    got = _rays(bg, sc, cuda)
    PR.compare(name, "kernel", sc, got, fg)
    if name == "empty cloud":
        assert not fg.any()
    else:
        assert fg.any(axis=(1, 2)).sum() >= min(sc["F"], 4)
    if name == "tile+1":
        assert sc["F"] == L.PLANE_CAM_TILE + 1 and fg[L.PLANE_CAM_TILE].any()


@pytest.mark.parametrize("name", list(PR.SPECIAL))
def test_special_batches(cuda, name):
    sc = PR.any_scene(name)
    bg = _bg(sc, cuda)
    got = _rays(bg, sc, cuda)
    PR.compare(name, "kernel", sc, got, _np(bg.fg_masks))
    if name == "parallel":     # every ray took the world origin: one answer, and not black
        assert got.any() and np.all(got == got[0])
    if name == "no view fits":
        assert not got.any()


def test_whole_frame_through_camera_rays(cuda):
    from pointnerf_amd import camera_rays
    sc = PR.named_scene("F5 uint8 frame")
    bg = _bg(sc, cuda)
    campos = torch.from_numpy(sc["campos"]).to(cuda)[None]
    rot = torch.from_numpy(sc["camrot"]).float().to(cuda)[None]
    img = bg.frame(campos, rot, sc["render_K"], sc["h"], sc["w"])
    assert img.shape == (1, sc["h"], sc["w"], 3)
    raydir = camera_rays(sc["render_K"], rot[0], sc["h"], sc["w"], device=cuda)
    assert np.array_equal(_np(raydir), sc["raydir"])             # the restatement's rays are camera_rays' rays
    assert torch.equal(img.reshape(1, -1, 3), bg.rays(campos, raydir))
    PR.compare("frame()", "kernel", sc, _np(img).reshape(-1, 3), _np(bg.fg_masks))


def test_corner_texels_bit_for_bit(cuda):
    """Rays built from the texels' own positions: the plane point lands exactly
    on (W-1, H-1) and the other corners, whose taps at x = W / y = H weigh
    nothing; a quarter texel outside the image there is no sample."""
    c = PR.corner_case()
    bg = _bg(c, cuda)
    assert not bg.fg_masks.any()
    got = _rays(bg, c, cuda)
    assert np.array_equal(got.view(np.uint32), c["want"].view(np.uint32)), (got, c["want"])
    # a point on that texel covers it (ceil of an integer is itself): the ray goes black, and so does
    # the ray at (W - 1.5, H - 1), which rounds up to the same texel
    pts = (c["campos"] + 4.0 * c["raydir"][[0]]).astype(np.float32)
    bg.refresh_fg(torch.from_numpy(pts))
    fg = _np(bg.fg_masks)
    assert fg.sum() == 1 and fg[0, c["H"] - 1, c["W"] - 1] == 1
    again = _rays(bg, c, cuda)
    assert not again[0].any() and not again[8].any() and np.array_equal(again[1:8], got[1:8])
    # (10.5, 7.25) rounds up to texel (11, 8)
    bg.refresh_fg(torch.from_numpy((c["campos"] + 4.0 * c["raydir"][[7]]).astype(np.float32)))
    fg = _np(bg.fg_masks)
    assert fg.sum() == 1 and fg[0, 8, 11] == 1
    assert not _rays(bg, c, cuda)[7].any()


def test_caller_masks_equal_built_masks(cuda):
    sc = PR.named_scene("F5 uint8 frame")
    built = _bg(sc, cuda)
    want = _rays(built, sc, cuda)
    for given in (built.fg_masks.clone(), built.fg_masks.bool().cpu().numpy()):
        mine = _bg(sc, cuda, fg_masks=given)
        assert torch.equal(mine.fg_masks, built.fg_masks)
        got = _rays(mine, sc, cuda)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # any masks the caller likes: the fp64 reference with exactly those
    rng = np.random.default_rng(4)
    own = rng.random((sc["F"], sc["H"], sc["W"])) < 0.3
    got = _rays(_bg(sc, cuda, fg_masks=own), sc, cuda)
    PR.compare("fg_masks= random", "kernel", sc, got, given_fg=own)


def test_outputs_stay_inside_their_buffers(cuda):
    """Direct calls on canary-filled buffers with tails."""
    sc = PR.named_scene("R257")
    fs = _frames(sc, cuda)
    F, H, W, R, tail = sc["F"], sc["H"], sc["W"], len(sc["raydir"]), 1024
    xyz = torch.from_numpy(sc["xyz"]).to(cuda)
    fg = torch.full((F * H * W + tail,), CANARY, dtype=torch.uint8, device=cuda)
    fg[:F * H * W] = 0
    lib, st = L.lib(), L.stream_ptr(cuda)
    for _ in range(2):
        L.check(lib.pnr_plane_fg_masks(L.ptr(xyz), xyz.shape[0], L.ptr(fs.cams), F, H, W, L.ptr(fg), F * H * W, st),
                "pnr_plane_fg_masks")
    assert torch.all(fg[F * H * W:] == CANARY)
    masks = fg[:F * H * W].reshape(F, H, W)
    assert np.array_equal(_np(masks), _np(_bg(sc, cuda).fg_masks))
    bg = torch.full((R * 3 + tail,), float("nan"), dtype=torch.float32, device=cuda)
    bg.view(torch.int32).fill_(0x7FC0A5A5)
    campos = torch.from_numpy(sc["campos"]).to(cuda)
    raydir = torch.from_numpy(sc["raydir"]).to(cuda)
    h3 = lambda v: (L.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    L.check(lib.pnr_plane_bg(L.ptr(campos), L.ptr(raydir), R, L.ptr(fs.images), 1, L.ptr(fs.cams), F, H, W,
                             L.ptr(fg), F * H * W, h3(sc["plane_pnt"]), h3(sc["plane_normal"]),
                             h3(sc["plane_color"]), L.ptr(bg), R, None, None, st), "pnr_plane_bg")
    assert torch.all(bg[R * 3:].view(torch.int32) == 0x7FC0A5A5)
    got = _np(bg[:R * 3]).reshape(R, 3)
    assert np.isfinite(got).all()                                  # every ray was written
    PR.compare("canary R257", "kernel", sc, got, _np(masks))
    # bad sizes are refused on the host
    assert lib.pnr_plane_bg(L.ptr(campos), L.ptr(raydir), R, L.ptr(fs.images), 1, L.ptr(fs.cams), F, H, W, L.ptr(fg),
                            F * H * W - 1, h3(sc["plane_pnt"]), h3(sc["plane_normal"]), h3(sc["plane_color"]),
                            L.ptr(bg), R, None, None, st) == L.PNR_EINVAL
    assert lib.pnr_plane_bg(L.ptr(campos), L.ptr(raydir), R, L.ptr(fs.images), 1, L.ptr(fs.cams), F, H, W, L.ptr(fg),
                            F * H * W, h3(sc["plane_pnt"]), h3(sc["plane_normal"]), h3(sc["plane_color"]),
                            L.ptr(bg), R - 1, None, None, st) == L.PNR_EINVAL
    assert lib.pnr_plane_fg_masks(L.ptr(xyz), xyz.shape[0], L.ptr(fs.cams), F, H, W, L.ptr(fg), F * H * W - 1,
                                  st) == L.PNR_EINVAL


# --------------------------------------------------------------------- epilogue
def test_fused_equals_rays_plus_fill(cuda):
    sc = PR.named_scene("F5 uint8 frame")
    bg = _bg(sc, cuda)
    R = len(sc["raydir"])
    campos = torch.from_numpy(sc["campos"]).to(cuda)[None]
    raydir = torch.from_numpy(sc["raydir"]).to(cuda)[None]
    gen = torch.Generator().manual_seed(3)
    color = torch.rand((1, R, 3), generator=gen).to(cuda)
    is_bg = torch.rand((1, R, 1), generator=gen).to(cuda)
    is_bg[0, ::3] = 1.0
    is_bg[0, 1::7] = 0.0
    bg_ray = bg.rays(campos, raydir)
    want = color + is_bg * bg_ray                                  # two fp32 roundings, as the kernel's
    outs = []
    for _ in range(2):
        c = color.clone()
        got_bg = bg.fused(campos, raydir, is_bg, c)
        assert torch.equal(got_bg, bg_ray)
        outs.append(c)
    assert torch.equal(outs[0], outs[1])
    ulps = PR.RR.ulp_distance(_np(outs[0]), _np(want)).max()
    print(f"fused vs rays + torch: {ulps} ulp, {int((bg_ray != 0).any(-1).sum())} rays with a background")
    assert ulps <= 1
    assert (bg_ray != 0).any() and not torch.equal(outs[0], color)


def test_module_forward_then_fill(cuda):
    from formula import UPSTREAM_SHAPES, formula_params
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    from scenes import scene
    psc = PR.named_scene("F5 uint8 frame")
    bg = _bg(psc, cuda)
    h, w = psc["h"], psc["w"]
    bg_ray = bg.rays(torch.from_numpy(psc["campos"]).to(cuda)[None], torch.from_numpy(psc["raydir"]).to(cuda)[None])
    sc = scene(8000, H=h, W=w, theta=40.0, shading_color_channel_num=3)
    agg = PointAggregator(sc["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in formula_params(UPSTREAM_SHAPES, salt=0.3).items()})
    pts = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                       torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]))
    model = NeuralPointsRayMarching(sc["opt"], pts, agg.eval())
    with torch.no_grad():
        out = model(campos=torch.from_numpy(sc["campos"]).to(cuda)[None],
                    raydir=torch.from_numpy(sc["raydir"]).to(cuda)[None],
                    camrotc2w=torch.from_numpy(sc["camrot"]).to(cuda)[None], near=torch.tensor([[2.0]], device=cuda),
                    far=torch.tensor([[6.0]], device=cuda), bg_ray=bg_ray)
    color, is_bg, hit = out["coarse_raycolor"].clone(), out["coarse_is_background"].clone(), out["ray_mask"][0] > 0
    assert color.shape == (1, h * w, 3) and 20 < int(hit.sum()) < h * w
    filled = bg.fill(out, bg_ray)
    assert filled is out
    got = out["coarse_raycolor"]
    assert torch.equal(got[0][~hit], bg_ray[0][~hit]), "a missed ray is not its bg_ray bit for bit"
    assert torch.equal(got[0][hit], (color + is_bg * bg_ray)[0][hit])
    assert (bg_ray[0][~hit] != 0).any() and (bg_ray[0][hit] != 0).any()


def test_fill_and_fused_refusals(cuda):
    from pointnerf_amd import PlaneBackground
    sc = PR.named_scene("R65")
    bg = _bg(sc, cuda)
    R = len(sc["raydir"])
    campos = torch.from_numpy(sc["campos"]).to(cuda)[None]
    raydir = torch.from_numpy(sc["raydir"]).to(cuda)[None]
    bg_ray = bg.rays(campos, raydir)
    is_bg = torch.ones((1, R, 1), device=cuda)
    wide = dict(coarse_raycolor=torch.zeros((1, R, 128), device=cuda), coarse_is_background=is_bg)
    with pytest.raises(L.PnrError, match="128 channels"):
        bg.fill(wide, bg_ray)
    with pytest.raises(L.PnrError, match="128 channels"):
        bg.fused(campos, raydir, is_bg, wide["coarse_raycolor"])
    grad = torch.zeros((1, R, 3), device=cuda, requires_grad=True)
    with pytest.raises(L.PnrError, match="is_bg gradient"):
        bg.fill(dict(coarse_raycolor=grad, coarse_is_background=is_bg), bg_ray)
    with pytest.raises(L.PnrError, match="is_bg gradient"):
        bg.fused(campos, raydir, is_bg, grad)
    with pytest.raises(L.PnrError, match="fg_masks must be"):
        _bg(sc, cuda, fg_masks=torch.zeros((sc["F"], sc["H"], sc["W"] + 1), dtype=torch.uint8))
    with pytest.raises(L.PnrError, match="one of them"):
        PlaneBackground(_frames(sc, cuda), sc["plane_pnt"], sc["plane_normal"], sc["plane_color"])
    with pytest.raises(L.PnrError, match="raydir must be"):
        bg.rays(campos, raydir[0, :, :2])


def test_near_plane(cuda):
    sc = PR.named_scene("F5 uint8 frame")
    bg = _bg(sc, cuda)
    n, p0 = sc["plane_normal"].astype(np.float64), sc["plane_pnt"].astype(np.float64)
    rng = np.random.default_rng(2)
    xyz = (p0 + rng.normal(0, 0.3, (500, 3))).astype(np.float32)
    want = np.abs(xyz.astype(np.float64) @ n - p0 @ n) < 0.2
    far = np.abs(np.abs(xyz.astype(np.float64) @ n - p0 @ n) - 0.2) > 1e-5
    got = _np(bg.near_plane(torch.from_numpy(xyz).to(cuda)))
    assert np.array_equal(got[far], want[far]) and 0 < want.sum() < 500
