"""The DTU scripts' aggregator flags (dtu_script_opt: 63-channel features assembled from
[colour, dir, conf, feat], agg_intrp_order 1; the ete script's order 2) end to end on the small
perspective scene of tests/pquery_scene.py (4000 points, 40 x 32): render_pixels against the chain
by hand, forward's routes against each other, a checkpoint round trip at width 63 and the
refusals (training, the point-growing probe, a bf16 table).  DESIGN.md section 31.

The chain by hand: the device's own query (NeuralPoints.forward's rows of pnr_pquery), the float64
restatement of tests/aggregate_dtu_ref.py on those samples, oracle.ray_dist and composite_ref's
march in float64, then the fill.  Bar: test_frame_vs_chain_by_hand's atol 2e-4, rtol 1e-4."""
import numpy as np
import pytest
import torch

import aggregate_dtu_ref as DR
import composite_ref as CR
from oracle import oracle as O
from pquery_scene import pscene
from test_gpu_pquery_frame import near, pixel_args
from test_gpu_pquery_render import inputs

pytestmark = pytest.mark.gpu
SALT = 0.2
_SCENES, _CHAIN = {}, {}


def scene(order, **over):
    """The scene with the scripts' aggregator flags; parts of the cloud: 56 features, colour, dir, conf."""
    from pointnerf_amd.options import DTU_SCRIPT, dtu_script_opt
    key = (order, tuple(sorted(over.items())))
    if key not in _SCENES:
        sc = pscene(**dict(DTU_SCRIPT, agg_intrp_order=order, **over))
        want = dtu_script_opt(agg_intrp_order=order)
        for k in DTU_SCRIPT:                      # the aggregator flags are dtu_script_opt()'s
            assert getattr(sc["opt"], k) == getattr(want, k), k
        n = len(sc["xyz"])
        g = torch.Generator().manual_seed(11)
        dirs = torch.randn((n, 3), generator=g)
        sc.update(feat=torch.rand((n, 56), generator=g) - 0.5, color=torch.rand((n, 3), generator=g),
                  dir=dirs / dirs.norm(dim=1, keepdim=True), conf=torch.rand((n, 1), generator=g),
                  bg=torch.rand(128, generator=torch.Generator().manual_seed(1)).numpy())
        _SCENES[key] = sc
    return _SCENES[key]


def make_model(sc, cuda, precision="fp32", **kw):
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    opt = sc["opt"]
    agg = PointAggregator(opt).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in DR.params_for(63, SALT).items()})
    tables = NeuralPoints.assemble_embedding(opt, sc["feat"], sc["color"], sc["dir"], sc["conf"])
    assert tables[0].shape[-1] == 63
    np_ = NeuralPoints(opt, cuda, torch.from_numpy(sc["xyz"]), *tables)
    return NeuralPointsRayMarching(opt, np_, agg.eval(), precision=precision, **kw)


def chain(order, cuda):
    """The frame by hand, once per order (float64 from the device's samples on)."""
    if order in _CHAIN:
        return _CHAIN[order]
    sc = scene(order)
    m = make_model(sc, cuda)
    inp = inputs(sc, cuda)
    with torch.no_grad():
        t = m.neural_points(dict({k: inp[k] for k in ("pixel_idx", "camrotc2w", "campos", "near", "far", "h", "w",
                                                        "intrinsic", "raydir")}, focal=None, gt_image=None))
    s_color, _rw, s_dir, s_conf, s_emb, s_pers, s_xyz, s_mask, s_loc, s_loc_w, s_dirs, ray_mask, vsize, _ = t
    assert s_emb.shape[-1] == 63
    n = lambda x: x[0].cpu().numpy()   # noqa: E731
    params = {k: v.astype(np.float64) for k, v in DR.params_for(63, SALT).items()}
    feats, rv, _, _ = DR.aggregate(params, n(s_color), None, n(s_dir), n(s_conf), n(s_emb), n(s_pers), n(s_xyz),
                                   n(s_mask), n(s_loc), n(s_loc_w), n(s_dirs), order=order, dtype=np.float64)
    rd = O.ray_dist(n(s_loc), rv, float(vsize[2]), sc["opt"].raydist_mode_unit)
    mr = CR.march_reference(torch.from_numpy(rd), torch.from_numpy(rv), torch.from_numpy(feats),
                            torch.from_numpy(sc["bg"]), torch.float64)
    rm = ray_mask[0].cpu().numpy()
    hit = rm > 0
    R = len(hit)
    want = dict(color=np.broadcast_to(sc["bg"][None].astype(np.float64), (R, 128)).copy(),
                opacity=np.zeros((R, sc["opt"].SR)), is_bg=np.ones(R), ray_mask=rm, valid=np.zeros(R, bool))
    want["color"][hit], want["opacity"][hit], want["is_bg"][hit] = mr["color"].numpy(), mr["opacity"].numpy(), mr["bgT"].numpy()
    want["valid"][hit] = rv.any(-1)
    assert hit.sum() > 300 and want["valid"].sum() > 200
    _CHAIN[order] = want
    return want


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "fp32h2"])
@pytest.mark.parametrize("order", [1, 2])
def test_render_pixels_vs_chain_by_hand(cuda, order, precision):
    sc = scene(order)
    want = chain(order, cuda)
    m = make_model(sc, cuda, precision)
    color, opacity, is_bg, ray_mask = (t.cpu().numpy() for t in m.render_pixels(*pixel_args(sc, inputs(sc, cuda))))
    assert m.h2_fallbacks == 0
    what = f"order {order} {precision}"
    assert ray_mask.dtype == np.int8 and np.array_equal(ray_mask, want["ray_mask"]), what
    d = np.abs(color - want["color"])
    print(f"{what}: colour max |d| {d.max():.3e}, over the bar {(d / (2e-4 + 1e-4 * np.abs(want['color']))).max():.4f}")
    near(color, want["color"], what + " colour")
    near(opacity, want["opacity"], what + " opacity")
    near(is_bg, want["is_bg"], what + " is_bg")
    if order == 1:      # raw2out_color: every composited channel inside the sigmoid's range (bg in [0, 1])
        assert color.min() > -0.0011 and color.max() < 1.0011
    empty = (want["ray_mask"] > 0) & ~want["valid"]
    for rows in (empty, want["ray_mask"] == 0):
        assert np.array_equal(color[rows], np.broadcast_to(sc["bg"], (int(rows.sum()), 128))), what
        assert (is_bg[rows] == 1).all() and (opacity[rows] == 0).all(), what
    assert m.last_counts["R_valid"] == int(want["valid"].sum())


@pytest.mark.parametrize("order", [1, 2])
def test_forward_routes_agree(cuda, order):
    """pixels (fused_perspective) and seams (the reference-shaped forward) of one perspective model, and the
    eval route of the same cloud under the world query against its own render_rays."""
    sc = scene(order, zero_one_loss_items=())             # no loss reads the aux outputs
    inp = inputs(sc, cuda)
    seams, pixels = make_model(sc, cuda), make_model(sc, cuda, fused_perspective=True)
    with torch.no_grad():
        want, got = seams(**inp), pixels(**inp)
    assert (seams.path, pixels.path) == ("seams", "pixels")
    assert set(got) == set(want)
    for k in ("ray_mask", "queried_shading"):
        assert torch.equal(got[k], want[k]), k
    for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "coarse_mask"):
        near(got[k].cpu().numpy(), want[k].cpu().numpy(), f"order {order} {k}")
    ch = chain(order, cuda)
    assert np.array_equal(want["ray_mask"][0].cpu().numpy(), ch["ray_mask"])
    near(want["coarse_raycolor"][0].cpu().numpy(), ch["color"], f"order {order} seams vs chain")
    # the world model of the same cloud and weights: forward's eval route is its render_rays
    from pointnerf_amd.options import DTU_SCRIPT
    wsc = dict(sc, opt=pscene(**dict(DTU_SCRIPT, agg_intrp_order=order, wcoord_query=1, zero_one_loss_items=()))["opt"])
    world = make_model(wsc, cuda)
    with torch.no_grad():
        out = world(**inp)
        color, opacity, is_bg, ray_mask = world.render_rays(inp["campos"][0], inp["camrotc2w"][0], inp["raydir"][0],
                                                            2.0, 6.0, inp["bg_color"])
    assert world.path == "eval" and ray_mask.any()
    assert torch.equal(out["ray_mask"][0], ray_mask)
    assert torch.equal(out["coarse_raycolor"][0], color) and torch.equal(out["coarse_point_opacity"][0], opacity)
    if order == 1:
        assert float(color.min()) > -0.0011 and float(color.max()) < 1.0011


def test_eval_route_precisions_agree(cuda):
    """render_rays of the world model at width 63, order 1: the three precisions against each other at the frame
    bar (the world query's samples are the same for all three)."""
    from pointnerf_amd.options import DTU_SCRIPT
    sc = scene(1)
    wsc = dict(sc, opt=pscene(**dict(DTU_SCRIPT, wcoord_query=1))["opt"])
    inp = inputs(sc, cuda)
    a = (inp["campos"][0], inp["camrotc2w"][0], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    outs = {}
    for precision in ("fp32", "fp32x3", "fp32h2"):
        m = make_model(wsc, cuda, precision)
        outs[precision] = [t.cpu().numpy() for t in m.render_rays(*a)]
        assert m.h2_fallbacks == 0
    for p in ("fp32x3", "fp32h2"):
        assert np.array_equal(outs[p][3], outs["fp32"][3])
        for x, y, k in zip(outs[p][:3], outs["fp32"][:3], ("colour", "opacity", "is_bg")):
            near(x, y, f"{p} vs fp32 {k}")
    assert outs["fp32"][3].sum() > 100          # the world grid marks fewer rays than the frustum query


def test_checkpoint_round_trip_renders_the_same_bits(cuda, tmp_path):
    from pointnerf_amd.checkpoint import grow_points, load_ray_marching, prune, save_ray_marching
    sc = scene(1)
    m = make_model(sc, cuda, "fp32")
    a = pixel_args(sc, inputs(sc, cuda))
    want = m.render_pixels(*a)
    path = str(tmp_path / "dtu_net_ray_marching.pth")
    save_ray_marching(m, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(sd["neural_points.points_embeding"].shape) == (1, 4000, 63)
    assert tuple(sd["aggregator.block1.0.weight"].shape) == (256, 501)
    m2 = load_ray_marching(path, sc["opt"], cuda)
    assert not m2.load_report["missing"] and not m2.load_report["unexpected"]
    m2.precision = "fp32"
    got = m2.render_pixels(*a)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.options import dtu_opt
    with pytest.raises(PnrError, match=r"63 wide.*point_features_dim is 32"):
        load_ray_marching(path, dtu_opt(), cuda)
    # prune and grow at width 63
    np_ = m2.neural_points
    dropped = prune(np_, 2.0)                        # default_conf 1 everywhere: every point goes
    assert dropped == 4000 and tuple(np_.points_embeding.shape) == (1, 0, 63)
    grow_points(np_, torch.rand((5, 3)), torch.rand((5, 63)), torch.rand((5, 3)), torch.rand((5, 3)), torch.rand((5, 1)))
    assert tuple(np_.points_embeding.shape) == (1, 5, 63) and np_.tables()[0].emb_dim == 63


def test_refusals_before_any_launch(cuda):
    """Training, the point-growing probe and a bf16 table raise PnrError naming the flag, before a launch."""
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.renderer import NeuralPoints
    sc = scene(1)
    inp = inputs(sc, cuda)
    a = (inp["campos"][0], inp["camrotc2w"][0], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    m = make_model(sc, cuda)
    with pytest.raises(PnrError, match="point_features_dim 63"):
        m.render_rays_train(*a)
    m.train()
    with pytest.raises(PnrError, match="point_features_dim 63"):
        m(**inp)                                     # grad mode, train(), trainable parameters: a training step
    m.eval()
    m.opt.prob = 1
    try:
        with pytest.raises(PnrError, match="prob == 1.*point_features_dim 63"):
            with torch.no_grad():
                m(**inp)
        with pytest.raises(PnrError, match="point_features_dim 63"):
            m.probe_maps(*a[:5], torch.zeros((a[2].shape[0], sc["opt"].SR), device=cuda))
    finally:
        m.opt.prob = 0
    assert m.last_counts is None and m.last_train_aux is None     # nothing was rendered
    # order 1 alone (width 32) is refused by the same paths, naming its flag
    from pointnerf_amd.aggregator import PointAggregator
    o32 = pscene(agg_intrp_order=1)["opt"]
    with pytest.raises(PnrError, match="agg_intrp_order 1"):
        PointAggregator(o32).to(cuda).packed_train(h2=True)
    with pytest.raises(PnrError, match="bf16"):
        NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.rand((1, 4000, 63)), emb_dtype=torch.bfloat16)
    with pytest.raises(PnrError, match="point_features_dim"):
        m.neural_points.tables(bf16=True)
    from pointnerf_amd.options import DTU_SCRIPT
    wsc = dict(sc, opt=pscene(**dict(DTU_SCRIPT, wcoord_query=1))["opt"])
    with pytest.raises(PnrError, match="bf16.*point_features_dim 63"):
        make_model(wsc, cuda, "bf16").render_rays(*a)
