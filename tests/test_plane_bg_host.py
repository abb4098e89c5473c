"""tests/plane_bg_ref.py on the CPU: its sampler is grid_sample's,
its fp32 twin stays inside every bar of tests/test_gpu_plane_bg.py on every
scene that test renders, and the fp64 reference alone keeps the banded rays
within the cap on each of them."""
import numpy as np
import pytest
import torch

import plane_bg_ref as PR

ALL_SCENES = list(PR.SCENES) + list(PR.SPECIAL)


def _grid_sample(im, u, v):
    """[N,3] float64: F.grid_sample(bilinear, zeros, align_corners=True) of one
    image [H,W,3] at the pixel positions (u, v), normalised as the reference
    does (mvs_utils.py:313-314)."""
    H, W, _ = im.shape
    gx = torch.from_numpy(u) / ((W - 1.0) / 2.0) - 1.0
    gy = torch.from_numpy(v) / ((H - 1.0) / 2.0) - 1.0
    grid = torch.stack([gx, gy], -1)[None, None]
    src = torch.from_numpy(im).permute(2, 0, 1)[None]
    out = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out[0, :, 0].T.numpy()


@pytest.mark.parametrize("name", ["F5 uint8 frame", "F5 float", "F5 per-frame K"])
def test_bilinear_is_grid_sample_with_integer_texel_centres(name):
    sc = PR.named_scene(name)
    H, W = sc["H"], sc["W"]
    ref = PR.evaluate(sc["campos"], sc["raydir"], sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], sc["cams"],
                      sc["images"], sc["fg64"])
    im = PR.images_as(sc["images"], np.float64)
    eps = 1e-7
    edge_u = np.array([W - 1, 0, W - 1, 0, W - 1 + eps, -eps, W - 1, 3.0, W - 1.5, W - 1 - eps, W - 0.5, -0.5, 4.0],
                      np.float64)
    edge_v = np.array([H - 1, 0, 0, H - 1, 5.0, 5.0, H - 1 + eps, -eps, H - 1, H - 1 - eps, 2.0, 2.0, H - 0.25],
                      np.float64)
    seen = 0
    for f in range(sc["F"]):
        inb = ref["inb"][:, f]
        u = np.concatenate([ref["u"][inb, f], edge_u])
        v = np.concatenate([ref["v"][inb, f], edge_v])
        got = PR.bilinear(im, f, u, v)
        want = _grid_sample(im[f], u, v)
        # grid_sample goes through the normalised coordinate and back: a few ulp of W in the position
        assert np.abs(got - want).max() <= 1e-12, (f, np.abs(got - want).max())
        seen += int(inb.sum())
        # the + 0.5 convention would be half a texel away
        assert np.abs(PR.bilinear(im, f, u - 0.5, v - 0.5) - want).max() > 1e-3
    assert seen > 100
    # exactly on the last texel the sample is that texel; the taps at x = W, y = H weigh nothing
    assert np.array_equal(PR.bilinear(im, 0, np.float64(W - 1), np.float64(H - 1)), im[0, H - 1, W - 1])


@pytest.mark.parametrize("name", ALL_SCENES)
def test_fp32_twin_stays_inside_every_bar(name):
    sc = PR.any_scene(name)
    twin, fg32 = PR.twin_of(sc)
    PR.compare(name, "twin", sc, twin["bg"], fg32)
    # outside the bands the twin takes every decision as fp64 does, view by view
    ref = PR.evaluate(sc["campos"], sc["raydir"], sc["plane_pnt"], sc["plane_normal"], sc["plane_color"], sc["cams"],
                      sc["images"], sc["fg64"])
    banded, _ = PR.bands(ref, sc["H"], sc["W"], sc["plane_color"], *sc["fg_range"])
    for k in ("hit", "inb", "covered", "used"):
        assert np.array_equal(twin[k][~banded], ref[k][~banded]), k


@pytest.mark.parametrize("name", ALL_SCENES)
def test_banded_share_of_the_reference_is_within_the_cap(name):
    sc = PR.any_scene(name)
    share, ref = PR.banded_share(sc)
    print(f"{name}: banded share {share:.4f} of {len(sc['raydir'])} rays")
    assert share <= PR.BAND_CAP


def test_scenes_exercise_what_they_are_for():
    sc = PR.named_scene("F5 uint8 frame")
    _, ref = PR.banded_share(sc)
    used = ref["used"]
    two = used.sum(1) >= 2
    spread = np.where(used[..., None], ref["sample"], np.nan)
    differ = two & (np.nanmax(np.where(two[:, None, None], spread, 0), 1)
                    != np.nanmin(np.where(two[:, None, None], spread, 0), 1)).any(-1)
    assert differ.sum() >= 20                                    # the per-channel max has something to choose from
    winners = {tuple(np.nanargmax(spread[r], 0)) for r in np.nonzero(differ)[0]}
    assert any(len(set(w)) > 1 for w in winners)                 # and takes different views per channel
    assert not used[:, PR.OFF_VIEW].any() and ref["inb"][:, PR.OFF_VIEW].any()   # the view that is off by 0.05
    assert (~ref["hit"]).sum() >= 5 and ref["covered"].any() and (~ref["inb"]).any()
    assert ref["used"][PR.LEAD_RAY].sum() >= 2 and ref["covered"][PR.LEAD_RAY].any()
    tile = PR.named_scene("tile+1")
    _, ref = PR.banded_share(tile)
    assert ref["used"][:, PR.TILE].any()                         # the camera past the LDS tile decides rays
    par = PR.any_scene("parallel")
    _, ref = PR.banded_share(par)
    assert not ref["hit"].any() and ref["used"].any(1).all() and not ref["p"].any()
    _, ref = PR.banded_share(PR.any_scene("no view fits"))
    assert not ref["bg"].any() and ref["inb"].any()


def test_corner_case_is_exact():
    c = PR.corner_case()
    fg = np.zeros((1, c["H"], c["W"]), bool)
    for dt in (np.float64, np.float32):
        e = PR.evaluate(c["campos"], c["raydir"], c["plane_pnt"], c["plane_normal"], c["plane_color"], c["cams"],
                        c["images"], fg, dt)
        assert np.array_equal(e["u"][:, 0], c["uv"][:, 0]) and np.array_equal(e["v"][:, 0], c["uv"][:, 1])
        assert e["inb"][:, 0].tolist() == [True, True, True, True, False, False, False, True, True, False, False]
    assert np.array_equal(e["bg"], c["want"])                    # the fp32 twin, bit for bit
    assert c["want"][:4].all() and not c["want"][4:7].any() and not c["want"][9:].any()


def test_mask_lookup_rounds_up():
    """ceil, not floor: a point at (10.5, 7.25) marks texel (11, 8)."""
    c = PR.corner_case()
    pts = (c["campos"].astype(np.float64) + 4.0 * c["raydir"][7].astype(np.float64))[None].astype(np.float32)
    fg = PR.fg_masks(pts, c["cams"], c["H"], c["W"])
    assert fg.sum() == 1 and fg[0, 8, 11]
    on_bound = (c["campos"].astype(np.float64) + 4.0 * c["raydir"][0].astype(np.float64))[None].astype(np.float32)
    fg = PR.fg_masks(on_bound, c["cams"], c["H"], c["W"])
    assert fg.sum() == 1 and fg[0, c["H"] - 1, c["W"] - 1]        # u = W - 1 is in bounds
