"""The perspective query behind NeuralPoints and the module forward
(wcoord_query 0): the 14-tuple's gathers, the eval forward
against the chain run by hand from the restatement's query output through the
oracle's aggregator and composite (the project's tolerance for that chain,
test_gpu_api.py: atol 2e-4, rtol 1e-4), the training forward, the jitter, and
the world-only fused paths."""
import numpy as np
import pytest
import torch

import pquery_ref as PR
from formula import formula_params
from oracle import oracle as O
from pquery_scene import pscene
from pointnerf_amd import synthetic as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def features(sc, seed=0):
    n = len(sc["xyz"])
    emb, color, dirs, conf = S.point_features(n, seed=seed, default_conf=None)
    sc.update(emb=emb.numpy(), color=color.numpy(), dir=dirs.numpy(), conf=conf.numpy(),
              bg=torch.rand(128, generator=torch.Generator().manual_seed(seed + 1)).numpy())
    return sc


def lone_point_scene(**over):
    """The scene plus one point alone in the frame's top-left corner, with a
    radius limit (8 pixel widths, measured after the NN = 2 scaling by depth):
    rays whose columns the query block marks but whose centres lie farther than
    the limit from every listed point keep ray_mask 1 without any neighbour."""
    sc = pscene(radius_limit_scale=8.0, **over)
    geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
    p = geo.shift + geo.svs * np.array([1.5, 1.5, 20.5], F32)      # voxel (1, 1, 20), perspective coordinates
    xyz_c = np.array([p[0] * p[2], p[1] * p[2], p[2]], np.float64)
    w = sc["camrot"].astype(np.float64) @ xyz_c + sc["campos"]
    sc["xyz"] = np.concatenate([sc["xyz"], w[None].astype(F32)])
    sc["pers"] = O.w2pers(sc["xyz"], sc["campos"], sc["camrot"])
    return features(sc)


def model(sc, cuda, params, train=False):
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    agg = PointAggregator(sc["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                       torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]))
    return NeuralPointsRayMarching(sc["opt"], np_, agg.train() if train else agg.eval(), precision="fp32")


def inputs(sc, cuda):
    raydir = S.pixel_rays(sc["H"], sc["W"], float(sc["intrinsic"][0, 0]), sc["camrot"])
    return dict(campos=torch.from_numpy(sc["campos"]).to(cuda)[None], raydir=torch.from_numpy(raydir).to(cuda)[None],
                bg_color=torch.from_numpy(sc["bg"]).to(cuda), camrotc2w=torch.from_numpy(sc["camrot"]).to(cuda)[None],
                pixel_idx=torch.from_numpy(sc["pixel_idx"]).to(cuda)[None].long(),
                near=torch.tensor([[2.0]], device=cuda), far=torch.tensor([[6.0]], device=cuda),
                h=torch.tensor([sc["H"]], device=cuda), w=torch.tensor([sc["W"]], device=cuda),
                intrinsic=torch.from_numpy(sc["intrinsic"]).to(cuda)[None])


def ref_query(sc):
    # the module's pers come from NeuralPoints.w2pers on the device; the restatement takes the oracle's
    return PR.query(sc["opt"], sc["pers"], sc["pixel_idx"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0,
                    sc["camrot"], sc["campos"])


@pytest.fixture(scope="module")
def lone():
    sc = lone_point_scene()
    return sc, ref_query(sc)


def device_pers(m, inp):
    return m.neural_points.w2pers(m.neural_points.xyz, inp["camrotc2w"], inp["campos"])[0].detach().cpu().numpy()


def test_neural_points_forward_14_tuple(cuda, lone):
    from pointnerf_amd._lib import PnrError
    sc, _ = lone
    m = model(sc, cuda, formula_params(salt=0.2))
    inp = inputs(sc, cuda)
    args = {k: inp[k] for k in ("pixel_idx", "camrotc2w", "campos", "near", "far", "h", "w", "intrinsic", "raydir")}
    with torch.no_grad():
        t = m.neural_points(dict(args, focal=None, gt_image=None))
    assert len(t) == 14
    s_color, s_rw, s_dir, s_conf, s_emb, s_pers, s_xyz, s_mask, s_loc, s_loc_w, s_dirs, ray_mask, vsize, _ = t
    # the restatement on the very perspective coordinates the module computed
    pers = device_pers(m, inp)
    q = PR.query(sc["opt"], pers, sc["pixel_idx"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0, sc["camrot"],
                 sc["campos"])
    pidx = torch.from_numpy(q["sample_pidx"]).long()
    assert np.array_equal(ray_mask[0].cpu().numpy(), q["ray_mask"]) and ray_mask.dtype == torch.int8
    assert np.array_equal(s_mask[0].cpu().numpy(), q["sample_pidx"] >= 0)
    assert np.array_equal(s_loc[0].cpu().numpy(), q["sample_loc"])
    idx = pidx.clamp(min=0).reshape(-1)
    shp = tuple(pidx.shape)
    for got, table, c in ((s_xyz, sc["xyz"], 3), (s_pers, pers, 3), (s_emb, sc["emb"], 32), (s_color, sc["color"], 3),
                          (s_dir, sc["dir"], 3), (s_conf, sc["conf"], 1)):
        want = torch.index_select(torch.from_numpy(np.ascontiguousarray(table)).reshape(-1, c), 0, idx).reshape(shp + (c,))
        assert torch.equal(got[0].cpu(), want)
    assert np.array_equal(vsize, q["vsize"])
    np.testing.assert_allclose(s_loc_w[0].cpu().numpy(), q["sample_loc_w"], atol=5e-6, rtol=0)
    np.testing.assert_allclose(s_dirs[0].cpu().numpy(), q["sample_ray_dirs"], atol=5e-6, rtol=0)
    for missing in ("pixel_idx", "h", "w", "intrinsic"):
        with pytest.raises(PnrError, match=missing):
            m.neural_points(dict(args, **{missing: None}))


def test_module_eval_forward_vs_chain_by_hand(cuda, lone):
    sc, _ = lone
    params = formula_params(salt=0.2)
    m = model(sc, cuda, params)
    inp = inputs(sc, cuda)
    with torch.no_grad():
        out = m(**inp)
    q = PR.query(sc["opt"], device_pers(m, inp), sc["pixel_idx"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0,
                 sc["camrot"], sc["campos"])
    pts = dict(xyz=sc["xyz"], emb=sc["emb"], color=sc["color"], dir=sc["dir"], conf=sc["conf"])
    g = O.gather(pts, q["sample_pidx"], sc["campos"], sc["camrot"])
    feats, rv, _, _ = O.aggregate(params, g["sampled_color"], None, g["sampled_dir"], g["sampled_conf"],
                                  g["sampled_embedding"], g["sampled_xyz_pers"], g["sampled_xyz"], g["sample_pnt_mask"],
                                  q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"])
    vz = float(q["vsize"][2])
    assert vz == F32(4.0 / 128)                    # the querier's (far - near) / z_depth_dim, not opt.vsize
    rd = O.ray_dist(q["sample_loc"], rv, vz, sc["opt"].raydist_mode_unit)
    color, _, opacity, _, _, bgT = O.ray_march(rd, rv, feats, sc["bg"])
    hit = q["ray_mask"] > 0
    R = len(hit)
    want_color = np.broadcast_to(sc["bg"][None], (R, 128)).copy()
    want_color[hit] = color
    want_op = np.zeros((R, sc["opt"].SR), F32)
    want_op[hit] = opacity
    want_bg = np.ones((R, 1), F32)
    want_bg[hit] = bgT
    want_qs = np.ones((R, 3), F32)
    want_qs[hit] = np.repeat((~rv.any(-1, keepdims=True)).astype(F32), 3, -1)
    assert set(out) == {"coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "coarse_mask",
                        "queried_shading", "ray_mask", "weight", "blend_weight", "conf_coefficient"}
    assert np.array_equal(out["ray_mask"][0].cpu().numpy(), q["ray_mask"])
    np.testing.assert_allclose(out["coarse_raycolor"][0].cpu().numpy(), want_color, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["coarse_point_opacity"][0].cpu().numpy(), want_op, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["coarse_is_background"][0].cpu().numpy(), want_bg, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["coarse_mask"][0].cpu().numpy(), 1 - want_bg, atol=2e-4, rtol=1e-4)
    assert np.array_equal(out["queried_shading"][0].cpu().numpy(), want_qs)
    # hit rays without any neighbour: ray_mask 1, the background's colour
    empty = np.nonzero(hit)[0][~rv.any(-1)]
    assert len(empty) > 0
    assert (out["ray_mask"][0].cpu().numpy()[empty] == 1).all()
    assert np.array_equal(out["coarse_raycolor"][0].cpu().numpy()[empty], np.broadcast_to(sc["bg"], (len(empty), 128)))
    assert (want_qs[empty] == 1).all() and (out["coarse_is_background"][0].cpu().numpy()[empty] == 1).all()


def test_module_forward_without_a_hit(cuda, lone):
    """A batch whose rays all miss: every row is fill_invalid's."""
    sc, q = lone
    miss = np.nonzero(q["ray_mask"] == 0)[0][:7]
    assert len(miss) == 7
    m = model(sc, cuda, formula_params(salt=0.2))
    inp = inputs(sc, cuda)
    inp["pixel_idx"] = inp["pixel_idx"][:, torch.from_numpy(miss).to(cuda)]
    inp["raydir"] = inp["raydir"][:, torch.from_numpy(miss).to(cuda)]
    with torch.no_grad():
        out = m(**inp)
    assert not out["ray_mask"].any() and out["coarse_point_opacity"].shape == (1, 7, sc["opt"].SR)
    assert np.array_equal(out["coarse_raycolor"][0].cpu().numpy(), np.broadcast_to(sc["bg"], (7, 128)))
    assert (out["coarse_is_background"] == 1).all() and (out["queried_shading"] == 1).all()


def test_module_train_forward_backward(cuda):
    sc = features(pscene(2000, SR=24))
    m = model(sc, cuda, formula_params(salt=0.7), train=True)
    m.train()
    out = m(**inputs(sc, cuda))
    assert out["coarse_raycolor"].requires_grad
    out["coarse_raycolor"][..., :3].square().mean().backward()
    grads = [("points_embeding", m.neural_points.points_embeding.grad), ("points_conf", m.neural_points.points_conf.grad)]
    grads += [(k, p.grad) for k, p in m.aggregator.named_parameters() if k.endswith("weight")]
    assert len(grads) > 5
    for name, gr in grads:
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0, name


def test_uniform_jitter_moves_depth_only(cuda):
    from pointnerf_amd._lib import PnrError
    from test_gpu_pquery import run
    sc = pscene(2000)
    base, _ = run(sc, cuda)
    sc["opt"].is_train, sc["opt"].shpnt_jitter = 1, "uniform"
    torch.manual_seed(3)
    jit, _ = run(sc, cuda)
    sc["opt"].shpnt_jitter = "passfunc"
    same, _ = run(sc, cuda)
    vz = float(base["vsize"][2])
    for k in ("sample_pidx", "ray_mask", "slot_z"):
        assert np.array_equal(jit[k], base[k]) and np.array_equal(same[k], base[k])
    assert np.array_equal(same["sample_loc"], base["sample_loc"])
    assert np.array_equal(jit["sample_loc"][..., :2], base["sample_loc"][..., :2])
    d = jit["sample_loc"][..., 2].astype(np.float64) - base["sample_loc"][..., 2]
    assert np.abs(d).max() <= vz / 2 + 6 * 2.0 ** -24 and np.abs(d).max() > vz / 4 and abs(d.mean()) < vz / 20
    w, _ = PR.pers2w(jit["sample_loc"], sc["camrot"], sc["campos"])
    np.testing.assert_allclose(jit["sample_loc_w"], w, atol=5e-6, rtol=0)
    sc["opt"].shpnt_jitter = "sideways"
    with pytest.raises(PnrError, match="shpnt_jitter"):
        run(sc, cuda)


def test_fused_frame_paths_are_world_only(cuda, lone):
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.render_eval import RenderGraph
    sc, _ = lone
    m = model(sc, cuda, formula_params(salt=0.2))
    inp = inputs(sc, cuda)
    a = (inp["campos"][0], inp["camrotc2w"][0], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    for call in (lambda: m.render_rays(*a), lambda: m.render_rays_train(*a), lambda: m.probe_rays(*a),
                 lambda: RenderGraph(m, *a),
                 lambda: m.render_camera(a[0], a[1], float(sc["intrinsic"][0, 0]), sc["H"], sc["W"], 2.0, 6.0, a[5])):
        with pytest.raises(PnrError, match="world-query only"):
            call()


@pytest.mark.parametrize("fused", [False, True])
def test_module_forward_takes_float_near_far(cuda, fused):
    """A perspective forward with Python-float near / far (and int h / w) equals the same call with
    tensors, on the seam route and the fused one."""
    sc = lone_point_scene(zero_one_loss_items=[])      # no aux output wanted: the fused route applies
    m = model(sc, cuda, formula_params(salt=0.2))
    m.fused_perspective = fused
    inp = inputs(sc, cuda)
    with torch.no_grad():
        want = m(**inp)
        assert m.path == ("pixels" if fused else "seams")
        got = m(**dict(inp, near=2.0, far=6.0, h=sc["H"], w=sc["W"]))
    assert set(got) == set(want) and want["ray_mask"].any()
    for k in want:
        assert torch.equal(got[k], want[k]), k
