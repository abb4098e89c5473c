"""pnr_camera_rays / pnr_ray_batch and pointnerf_amd.rays against the numpy
restatement tests/rays_ref.py.

Rule: everything the contract fixes is compared bit for bit -- the picks, the
frame, the coin, the directions without dir_norm, the gathered colours, the
renders and the training step they feed.  Two comparisons allow one fp32 ulp:
against synthetic.pixel_rays (its fp64 products are summed by BLAS, in an order
that is not the contract's) and with dir_norm (the device's fp64 sqrt and
division are not assumed to round like numpy's)."""
import gc

import numpy as np
import pytest
import torch

import rays_ref as RR
from pointnerf_amd import synthetic as S
from scenes import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _collect_models():
    """A training-mode model sits in a reference cycle, so its grid handle waits
    for the collector (test_gpu_loss.py does the same): free this module's
    model and the step scene it shares when the module is done, pass or fail."""
    yield
    import test_gpu_loss
    from pointnerf_amd import querier as Q
    test_gpu_loss._STEP.clear()
    gc.collect()
    Q.release_deferred()


F, H, W = 3, 7, 5          # H != W: an x/y or row/column swap cannot pass
SEED = 11
_SET = {}


def _set():
    """Three 7 x 5 frames with per-frame intrinsics (fx != fy, cx != W/2), made once."""
    if not _SET:
        rng = np.random.default_rng(5)
        _SET["u8"] = rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
        _SET["f32"] = rng.random(size=(F, H, W, 3), dtype=np.float32)
        cams = [S.camera(20.0 + 70.0 * f, -30.0 + 7.0 * f, 4.0 + 0.25 * f) for f in range(F)]
        _SET["campos"] = np.stack([c[0] for c in cams])
        _SET["camrot"] = np.stack([c[1] for c in cams])
        _SET["K"] = np.stack([np.array([[6.9 + f, 0, 2.3 + 0.1 * f], [0, 7.7 - f, 3.6 - 0.2 * f], [0, 0, 1]])
                              for f in range(F)])
        _SET["rows"] = np.stack([RR.cam_row(_SET["campos"][f], _SET["camrot"][f], _SET["K"][f]) for f in range(F)])
    return _SET


def _frame_set(cuda, kind="u8", bg="random", per_frame=True, **kw):
    from pointnerf_amd.rays import FrameSet
    s = _set()
    return FrameSet(s[kind], (s["campos"], s["camrot"]), s["K"] if per_frame else s["K"][0], 2.0, 6.0,
                    bg_color=bg, seed=SEED, device=cuda, **kw)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} entries differ"


# ------------------------------------------------------------------ directions
def test_camera_rays_bitwise(cuda):
    from pointnerf_amd.rays import camera_rays
    s = _set()
    for f in range(F):          # the full 7 x 5 frame, per-frame intrinsics
        got, pix = camera_rays(s["K"][f], s["camrot"][f], H, W, device=cuda, return_pixels=True)
        px, py = RR.picks("full", 0, 0, H, W)
        assert got.shape == (H * W, 3) and pix.shape == (H * W, 2)
        _same(pix, np.stack([px, py], -1).astype(np.float32), f"frame {f} pixel_idx")
        _same(got, RR.directions(px, py, s["rows"][f]), f"frame {f} raydir")
    focal = S.lego_focal(800) * 24 / 800.0      # a focal length, 24 x 24: 576 rays, three blocks
    row = RR.cam_row(np.zeros(3), s["camrot"][1], RR.focal_K(focal, 24, 24))
    px, py = RR.picks("full", 0, 0, 24, 24)
    _same(camera_rays(focal, torch.from_numpy(s["camrot"][1]).to(cuda), 24, 24), RR.directions(px, py, row), "24x24")
    rng = np.random.default_rng(1)              # explicit lists: 1 and 100 pixels, some between pixel centres
    for R in (1, 100):
        pixels = np.stack([rng.integers(0, W, R), rng.integers(0, H, R)], -1).astype(np.float32)
        pixels[::3] += rng.random((len(pixels[::3]), 2), dtype=np.float32)
        got, pix = camera_rays(s["K"][2], s["camrot"][2], H, W, pixels=pixels, device=cuda, return_pixels=True)
        _same(pix, pixels, f"list {R} pixel_idx")
        _same(got, RR.directions(pixels[:, 0], pixels[:, 1], s["rows"][2]), f"list {R} raydir")


def test_camera_rays_vs_pixel_rays(cuda):
    from pointnerf_amd.rays import camera_rays
    _, camrot = S.camera(40.0, -30.0, 4.0)
    focal = S.lego_focal(800) * 24 / 800.0
    got = camera_rays(focal, camrot, 24, 24, device=cuda).cpu().numpy()
    ref = S.pixel_rays(24, 24, focal, camrot)
    d = RR.ulp_distance(got, ref)
    print(f"camera_rays vs pixel_rays 24x24: {int((d > 0).sum())} of {d.size} entries differ, largest {int(d.max())} ulp")
    assert d.max() <= 1


def test_camera_rays_dir_norm(cuda):
    from pointnerf_amd.rays import camera_rays
    s = _set()
    worst = 0
    for f, (h, w) in ((0, (H, W)), (1, (24, 24))):
        got = camera_rays(s["K"][f], s["camrot"][f], h, w, dir_norm=True, device=cuda).cpu().numpy()
        px, py = RR.picks("full", 0, 0, h, w)
        ref = RR.directions(px, py, s["rows"][f], dir_norm=True)
        assert np.abs(np.linalg.norm(ref.astype(np.float64), axis=-1) - 1).max() < 2e-5
        worst = max(worst, int(RR.ulp_distance(got, ref).max()))
    print(f"dir_norm: largest distance {worst} ulp")
    assert worst <= 1


# --------------------------------------------------------------------- batches
CASES = [("random", 1), ("random", 10), ("random", 24), ("patch", 2), ("patch", 5), ("full", None)]


def _check_item(fs, item, mode, size, step, kind, frame=None):
    """One item against the restatement of (SEED, step)."""
    from pointnerf_amd.rays import camera_rays
    s = _set()
    px, py = RR.picks(mode, SEED, step, H, W, size)
    _, white, drawn = RR.batch_draw(SEED, step, F, H, W)
    f = drawn if frame is None else frame
    R = px.shape[0]
    what = f"{mode} {size} {kind} step {step}"
    assert item["id"].dtype == torch.int32 and item["id"].cpu().tolist() == [f], what
    assert item["pixel_idx"].shape == (1, R, 2) and item["raydir"].shape == (1, R, 3), what
    assert item["gt_image"].shape == (1, R, 3) and item["bg_color"].shape == (1, 3), what
    _same(item["pixel_idx"][0], np.stack([px, py], -1).astype(np.float32), what + " pixel_idx")
    _same(item["bg_color"], np.full((1, 3), 1.0 if white else 0.0, np.float32), what + " bg_color")
    rays = camera_rays(s["K"][f], s["camrot"][f], H, W, pixels=item["pixel_idx"][0], device=item["id"].device)
    _same(item["raydir"][0], rays, what + " raydir")
    _same(item["raydir"][0], RR.directions(px, py, s["rows"][f]), what + " raydir vs restatement")
    img = s[kind][f, py, px]
    gt = img.astype(np.float32) / np.float32(255.0) if kind == "u8" else img
    _same(item["gt_image"][0], gt, what + " gt_image")
    _same(item["campos"], s["campos"][f][None], what + " campos")
    _same(item["camrotc2w"], s["camrot"][f][None], what + " camrotc2w")
    _same(item["intrinsic"], s["K"][f].astype(np.float32)[None], what + " intrinsic")
    assert (item["near"], item["far"], item["h"], item["w"]) == (2.0, 6.0, H, W)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("mode,size", CASES)
def test_sample_matches_restatement(cuda, mode, size, kind):
    fs = _frame_set(cuda, kind)
    assert fs.step == 0 and fs.seed == SEED
    for step in (0, 1, 2, 2 ** 32 + 5):       # the last puts the counter's high word in use
        if step > 2:
            fs.step = step
        item = fs.sample(size, mode=mode)
        _check_item(fs, item, mode, size, step, kind)
        assert fs.step == step + 1


def test_three_ways_to_give_the_frame_agree(cuda):
    fs = _frame_set(cuda)
    step = 4
    _, _, drawn = RR.batch_draw(SEED, step, F, H, W)
    items = []
    for frame in (None, drawn, torch.tensor([drawn], dtype=torch.int32, device=cuda)):
        fs.step = step
        items.append(fs.sample(10, frame=frame))
        assert fs.step == step + 1
    _check_item(fs, items[0], "random", 10, step, "u8")
    for other in items[1:]:
        for k, v in items[0].items():
            assert torch.equal(v, other[k]) if torch.is_tensor(v) else v == other[k], k
    # a frame that was not drawn: the same picks on another image and camera
    fs.step = step
    _check_item(fs, fs.sample(10, frame=(drawn + 1) % F), "random", 10, step, "u8", frame=(drawn + 1) % F)
    # an evaluation frame does not move the training counter
    full = fs.frame(2)
    assert fs.step == step + 1 and full["id"].cpu().tolist() == [2] and full["raydir"].shape == (1, H * W, 3)
    _same(full["gt_image"][0], _set()["u8"][2].reshape(-1, 3).astype(np.float32) / np.float32(255.0), "frame(2)")
    fr = list(fs.probe_frames([1]))[0]
    assert fr["raydir"].shape == (H * W, 3) and fr["gt_image"].shape == (H * W, 3) and (fr["h"], fr["w"]) == (H, W)
    # a caller's background of any channel count passes through
    bg = torch.rand(128, device=cuda, requires_grad=True)
    it = _frame_set(cuda, bg=bg).sample(2, mode="patch")
    assert it["bg_color"].shape == (1, 128) and it["bg_color"].data_ptr() == bg.data_ptr()
    assert it["bg_color"].requires_grad


# --------------------------------------------------------------------- renders
def _model(sc, cuda, params):
    from test_gpu_train_contract import _model as contract_model
    return contract_model(sc, cuda, params)


def test_render_camera_equals_render_rays(cuda):
    from formula import formula_params
    from pointnerf_amd.rays import camera_rays
    sc = scene(8000, H=24, W=24)
    focal = S.lego_focal(800) * (24 / 800.0)
    dirs = camera_rays(focal, sc["camrot"], 24, 24, device=cuda)
    ref_dirs = torch.from_numpy(sc["raydir"]).to(cuda)
    differ = int((_bits(dirs) != _bits(ref_dirs)).sum())
    assert differ == 0, (f"{differ} of {dirs.numel()} direction entries differ from synthetic.pixel_rays: "
                         "the renders are not compared")
    m = _model(sc, cuda, formula_params(salt=0.35))
    campos, camrot = torch.from_numpy(sc["campos"]).to(cuda), torch.from_numpy(sc["camrot"]).to(cuda)
    bg = torch.from_numpy(sc["bg"]).to(cuda)
    want = m.render_rays(campos, camrot, ref_dirs, 2.0, 6.0, bg)
    got = m.render_camera(campos, camrot, focal, 24, 24, 2.0, 6.0, bg)
    assert int(want[3].sum()) > 20
    for g, w, name in zip(got, want, ("colour", "opacity", "is_bg", "ray_mask")):
        assert torch.equal(g, w), name


def test_finetune_step_fed_by_frame_set(cuda):
    """The same step twice: inputs from FrameSet.sample, then the same tensors
    built on the host -- loss and every gradient bit for bit.

    This holds only if the step itself is repeatable.  It was not for d
    points_conf while k_pairs_bwd added the pairs' terms into the point rows
    with float atomics (2-3 of 20 000 entries differed by up to 9e-13 between
    any two steps, whatever fed them); the terms are now written per pair and
    added per point in pair order (pnr_pairs_to_points_conf).  The third step
    below, fed by the host tensors again, prints the host-against-host figure
    next to the one under test if any gradient differs."""
    from pointnerf_amd.losses import RenderLoss
    from pointnerf_amd.rays import FrameSet
    from test_gpu_loss import _step_scene
    from test_gpu_train_contract import _inputs
    from test_gpu_train_contract import _model as contract_model
    sc, params, gt = _step_scene()
    focal = S.lego_focal(800) * (24 / 800.0)
    bg = torch.from_numpy(sc["bg"]).to(cuda)
    fs = FrameSet(gt.reshape(1, 24, 24, 3), (sc["campos"][None], sc["camrot"][None]), RR.focal_K(focal, 24, 24),
                  2.0, 6.0, bg_color=bg, device=cuda)
    item = fs.sample(mode="full", frame=0)
    host = _inputs(sc, cuda)
    _same(item["raydir"], host["raydir"], "raydir")
    _same(item["gt_image"], gt, "gt_image")
    _same(item["campos"], host["campos"], "campos")
    _same(item["camrotc2w"], host["camrotc2w"], "camrotc2w")
    m = contract_model(sc, cuda, params, train=True)
    m.train()
    rl = RenderLoss(sc["opt"])
    runs = []
    for feed, target in ((item, item["gt_image"]), (host, gt.to(cuda)), (host, gt.to(cuda))):
        m.zero_grad(set_to_none=True)
        out = m(**feed)
        total, _ = rl(out, target, model=m)
        total.backward()
        runs.append((total.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()
                                              if p.grad is not None}))
    assert float(runs[0][0]) > 0 and len(runs[0][1]) > 10
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert sorted(runs[0][1]) == sorted(runs[1][1])
    assert sum(bool(g.any()) for g in runs[0][1].values()) > 10
    differ = []
    for k, g in runs[0][1].items():
        assert torch.isfinite(g).all(), k
        d, dh = (g - runs[1][1][k]).abs(), (runs[1][1][k] - runs[2][1][k]).abs()
        if not torch.equal(g, runs[1][1][k]) or not torch.equal(runs[1][1][k], runs[2][1][k]):
            print(f"d {k}: FrameSet vs host {int((d > 0).sum())} of {d.numel()} entries differ, largest "
                  f"{float(d.max()):.3e}; host vs host {int((dh > 0).sum())} entries, largest {float(dh.max()):.3e}; "
                  f"largest entry {float(g.abs().max()):.3e}")
        if not torch.equal(g, runs[1][1][k]):
            differ.append(k)
    assert not differ, f"gradients not bit-equal between the two feeds: {differ}"


# ------------------------------------------------------------- no host, graphs
@pytest.mark.parametrize("frame", ["drawn", "device"])
def test_sample_reads_nothing_on_the_host(cuda, capsys, frame):
    fs = _frame_set(cuda)
    fr = None if frame == "drawn" else torch.tensor([1], dtype=torch.int32, device=cuda)
    batch = fs.sample(10, frame=fr)           # first call: the library, the tensors
    ran_debug = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        ran_debug = True
    except Exception as e:    # this torch build has no sync debug mode on ROCm
        print("set_sync_debug_mode unavailable:", repr(e))
    try:
        again = fs.sample(10, frame=fr, out=batch)
    finally:
        if ran_debug:
            torch.cuda.set_sync_debug_mode("default")
    assert again is batch
    _check_item(fs, batch, "random", 10, 1, "u8", frame=None if fr is None else 1)
    assert fs.step == 2
    with capsys.disabled():
        print(f"\n[no-host-read] FrameSet.sample(out=batch), frame {frame}; sync debug mode 'error' around it: "
              f"{'ran' if ran_debug else 'not available'}")


@pytest.mark.parametrize("mode,size", [("random", 24), ("patch", 2)])
def test_graph_capture_replays_the_next_batches(cuda, mode, size):
    """sample(out=batch) alone, captured on a side stream (a linear graph):
    three replays give the bits of eager steps s, s + 1, s + 2."""
    fs = _frame_set(cuda)
    s0 = 7
    fs.step = s0
    keys = ("raydir", "pixel_idx", "gt_image", "campos", "camrotc2w", "bg_color", "id", "intrinsic")
    eager = []
    batch = None
    for _ in range(3):
        batch = fs.sample(size, mode=mode, out=batch)
        eager.append({k: batch[k].clone() for k in keys})
    assert fs.step == s0 + 3
    assert not torch.equal(eager[0]["pixel_idx"], eager[1]["pixel_idx"])
    fs.step = s0
    for k in keys:
        batch[k].zero_()
    side = torch.cuda.Stream(cuda)
    torch.cuda.synchronize()
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            fs.sample(size, mode=mode, out=batch)
    finally:
        if gc_was_on:
            gc.enable()
    for n in range(3):
        g.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(batch[k], eager[n][k]), (n, k)
    assert fs.step == s0 + 3
