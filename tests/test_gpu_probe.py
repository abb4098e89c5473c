"""pnr_probe and the opt.prob == 1 outputs of NeuralPointsRayMarching.forward
(models/neural_points_volumetric_model_ori.py:351-372) against the fp64
restatement tests/probe_ref.py, on the same inputs: the query is bit-exact to
the CPU oracle, so the oracle's rows line up with the kernel's.

Rule (probe_ref.compare): ray_max_shading_opacity and ray_max_sample_loc_w are
copies and must be bit-equal (they imply s*, ties to the lowest slot); far_dist
and the averages may differ from fp64 by at most 4x the error of the same
restatement run in fp32, plus one ulp of the tensor's maximum.  No ray is left
out.  Measured on MI355X (max error / fp32 twin's max error): see DESIGN.md
"Point-growing probe"."""
import gc

import numpy as np
import pytest
import torch

import probe_ref as PR
from formula import formula_params
from scenes import flag_scene, oracle_points, scene

pytestmark = pytest.mark.gpu

SALT = 0.35
_CACHE = {}


def _scene(name):
    if name == "lego":
        return scene(20000, H=24, W=24, theta=40)
    if name == "scene101":
        return flag_scene("scene101", H=24)
    if name in ("k4", "k16"):
        return scene(20000, H=24, W=24, theta=40, K=int(name[1:]))
    if name == "rolled":   # point 0 = an interior surface point (the ground slab's points come last)
        sc = scene(20000, H=24, W=24, theta=40)
        for k in ("xyz", "emb", "color", "dir", "conf"):
            sc[k] = np.ascontiguousarray(np.roll(sc[k], -5000, axis=0))
        return sc
    raise KeyError(name)


def _ref(name):
    """(scene, oracle inputs) of a named scene, computed once and never modified."""
    if name not in _CACHE:
        sc = _scene(name)
        oi = PR.oracle_inputs(sc["opt"], oracle_points(sc), formula_params(salt=SALT), sc["campos"], sc["camrot"],
                              sc["raydir"], sc["bg"])
        _CACHE[name] = (sc, oi)
    return _CACHE[name]


def _points(sc, cuda, **kw):
    from pointnerf_amd.renderer import NeuralPoints
    return NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                        torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]),
                        **kw)


class _Probe:
    """pnr_query of a scene, then pnr_probe calls on uploaded opacities."""

    def __init__(self, sc, np_, cuda):
        from pointnerf_amd.querier import camera_tables
        self.dev, self.np_ = cuda, np_
        opt = sc["opt"]
        self.R, self.SR = sc["raydir"].shape[0], opt.SR
        self.cp, self.cr = camera_tables(torch.from_numpy(sc["campos"]).to(cuda),
                                         torch.from_numpy(sc["camrot"]).to(cuda))
        self.xyz = np_.xyz.detach().contiguous()
        self.bufs, _, self.rays, self.qp = np_.querier.run(self.xyz, torch.from_numpy(sc["raydir"]).to(cuda),
                                                           self.cp, self.cr, float(opt.near_plane),
                                                           float(opt.far_plane))
        self.pts, self._keep = np_.tables(self.cp, self.cr, bf16=True)
        have = dict(shading_avg_color=np_.points_color, shading_avg_dir=np_.points_dir,
                    shading_avg_conf=np_.points_conf)
        chans = (1, 3, 1, 3, 3, 1, 32)
        self.out = {k: None if have.get(k, 1) is None else
                    torch.full((self.R, c), float("nan"), dtype=torch.float32, device=cuda)
                    for k, c in zip(PR.KEYS, chans)}

    def ray_mask(self):
        return (self.bufs.ray_vcnt[:self.R] > 0).cpu().numpy()

    def launch(self, op_dev):
        from pointnerf_amd import _lib as L
        L.check(L.lib().pnr_probe(L.ctypes.byref(self.rays), L.ctypes.byref(self.qp), L.ctypes.byref(self.bufs.c),
                                  L.ctypes.byref(self.pts), L.ptr(op_dev), *(L.ptr(self.out[k]) for k in PR.KEYS),
                                  L.stream_ptr(self.dev)), "pnr_probe")

    def run(self, opacity):
        op = torch.from_numpy(np.ascontiguousarray(opacity, np.float32)).to(self.dev)
        self.launch(op)
        torch.cuda.synchronize()
        return {k: None if v is None else v.cpu().numpy() for k, v in self.out.items()}


def _planted(oi, SR):
    """A copy of the oracle's opacity [R,SR] with the cases the issue asks for:
    a few hit rays zeroed (s* = 0), a ray's maximum copied into an earlier and a
    later slot, and -- SR > 64 -- a tie across the two slots of one lane and a
    maximum in a slot of the second half (unfilled: no neighbour at all)."""
    op = oi["opacity"].copy()
    hit = np.nonzero(oi["q"]["ray_mask"] > 0)[0]
    for r in (hit[0], hit[len(hit) // 3], hit[-1]):
        op[r] = 0.0
    s0 = op[hit].argmax(-1)
    r = hit[np.nonzero((s0 >= 1) & (s0 <= SR - 2) & (op[hit].max(-1) > 0))[0][0]]
    s = int(op[r].argmax())
    op[r, s // 2] = op[r, s + 1] = op[r, s]
    if SR > 64:
        r = hit[len(hit) // 2]
        op[r, 3] = op[r, 67] = op[r].max() * 2 + 0.25
        r = hit[len(hit) // 2 + 1]
        op[r, SR - 5] = 0.5
    return op, hit


def _check(got, oi, op, what, emb_table=None):
    a = (oi["q"], oi["g"], oi["w"], oi["confc"], op)
    r64 = PR.probe_maps_ref(*a, dtype=np.float64, emb_table=emb_table)
    r32 = PR.probe_maps_ref(*a, dtype=np.float32, emb_table=emb_table)
    miss = oi["q"]["ray_mask"] == 0
    for k in PR.KEYS:
        if got[k] is not None:
            assert not np.isnan(got[k]).any(), f"{what} {k}: unwritten rows"
            assert not got[k].reshape(miss.shape[0], -1)[miss].any(), f"{what} {k}: ray_mask == 0 rows not zero"
    PR.compare(got, r64, r32, what=what)
    return r64


@pytest.mark.parametrize("name", ["lego", "scene101", "k4", "k16"])
def test_kernel_matches_restatement(name, cuda):
    sc, oi = _ref(name)
    pr = _Probe(sc, _points(sc, cuda), cuda)
    assert np.array_equal(pr.ray_mask(), oi["q"]["ray_mask"] > 0)
    SR = sc["opt"].SR
    # the oracle's own opacities (ties included: on the lego scene 65 of the 222 hit rays
    # have their two largest opacities equal), then the planted cases
    assert (oi["q"]["ray_mask"] > 0).sum() > 20
    _check(pr.run(oi["opacity"]), oi, oi["opacity"], name)
    op, hit = _planted(oi, SR)
    r64 = _check(pr.run(op), oi, op, name + " planted")
    assert r64["s_star"][hit[0]] == 0 and r64["s_star"][hit[-1]] == 0
    if SR > 64:
        assert r64["s_star"][hit[len(hit) // 2]] == 3 and r64["s_star"][hit[len(hit) // 2 + 1]] == SR - 5


def test_lego_scene_has_ties():
    """The reason the tie rule is pinned: the oracle's opacities tie often."""
    _, oi = _ref("lego")
    top = np.sort(oi["opacity"][oi["q"]["ray_mask"] > 0], -1)
    assert (top[:, -1] == top[:, -2]).sum() >= 10


def test_point0_clamp(cuda):
    """Empty neighbour slots gather point 0 (neural_points.py:790) in far_dist and
    the averages; with the cloud rolled, point 0 is an interior surface point."""
    sc, oi = _ref("rolled")
    pr = _Probe(sc, _points(sc, cuda), cuda)
    assert np.array_equal(pr.ray_mask(), oi["q"]["ray_mask"] > 0)
    r64 = _check(pr.run(oi["opacity"]), oi, oi["opacity"], "rolled")
    s = r64["s_star"][oi["q"]["ray_mask"] > 0]
    pid = oi["q"]["sample_pidx"][np.arange(s.shape[0]), s]
    assert (pid < 0).any(-1).sum() >= 1


def test_bf16_embedding_table(cuda):
    sc, oi = _ref("lego")
    np_ = _points(sc, cuda, emb_dtype=torch.bfloat16)
    pr = _Probe(sc, np_, cuda)
    assert pr.pts.emb_bf16 and not pr.pts.emb
    table = torch.from_numpy(sc["emb"]).to(torch.bfloat16).float().numpy()
    assert not np.array_equal(table, sc["emb"])
    op, _ = _planted(oi, sc["opt"].SR)
    _check(pr.run(op), oi, op, "bf16 table", emb_table=table)


def test_graph_capture_replays_bit_equal(cuda):
    """One launch, no sync, no allocation: pnr_probe alone captured on a side
    stream (a linear graph) replays to the eager call's bits."""
    sc, oi = _ref("lego")
    pr = _Probe(sc, _points(sc, cuda), cuda)
    op, _ = _planted(oi, sc["opt"].SR)
    eager = pr.run(op)
    op_dev = torch.from_numpy(op).to(cuda)
    for v in pr.out.values():
        v.fill_(float("nan"))
    side = torch.cuda.Stream(cuda)
    torch.cuda.synchronize()
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            pr.launch(op_dev)
    finally:
        if gc_was_on:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    for k in PR.KEYS:
        assert np.array_equal(pr.out[k].cpu().numpy().view(np.uint32), eager[k].view(np.uint32)), k


# ----------------------------------------------------------------- module level
def _boosted_params():
    """Opacities that reach the growing thresholds: alpha bias + 300 (CPU oracle:
    median of the per-ray maximum 0.62, largest 0.70)."""
    p = dict(formula_params(salt=SALT))
    p["alpha_branch.0.bias"] = p["alpha_branch.0.bias"] + 300
    return p


def _model(sc, cuda, params):
    from test_gpu_train_contract import _model as contract_model
    return contract_model(sc, cuda, params)


def _inputs(sc, cuda):
    from test_gpu_train_contract import _inputs as contract_inputs
    return contract_inputs(sc, cuda)


def test_module_forward_prob(cuda):
    sc, oi = _ref("lego")
    m = _model(sc, cuda, _boosted_params())
    R, SR = sc["raydir"].shape[0], sc["opt"].SR
    assert sc["opt"].prob == 0
    with torch.no_grad():
        out0 = m(**_inputs(sc, cuda))
        sc["opt"].prob = 1
        try:
            out1 = m(**_inputs(sc, cuda))
        finally:
            sc["opt"].prob = 0
    shapes = dict(zip(PR.KEYS, (1, 3, 1, 3, 3, 1, 32)))
    for k, c in shapes.items():
        assert k not in out0
        assert tuple(out1[k].shape) == (1, R, c) and out1[k].dtype == torch.float32, k
    assert set(out1) - set(out0) == set(PR.KEYS)
    for k, v in out0.items():
        assert torch.equal(v, out1[k]) if torch.is_tensor(v) else v == out1[k], k
    op = out1["coarse_point_opacity"][0].cpu().numpy()
    assert np.median(op[oi["q"]["ray_mask"] > 0].max(-1)) > 0.3
    got = {k: out1[k][0].cpu().numpy() for k in PR.KEYS}
    _check(got, oi, op, "module prob=1")
    # training mode has no probe (the reference probes under model.test())
    from pointnerf_amd._lib import PnrError
    sc["opt"].prob = 1
    try:
        m.train()
        with pytest.raises(PnrError, match="prob"):
            m(**_inputs(sc, cuda))
    finally:
        sc["opt"].prob = 0
        m.eval()


def test_module_absent_tables_and_probe_rays_chunks(cuda):
    """A cloud without colour / dir / conf tables gives None for their averages
    (conf_coefficient 1); probe_rays in ray chunks equals the one-batch call."""
    sc, oi = _ref("lego")
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    m = _model(sc, cuda, _boosted_params())
    inp = _inputs(sc, cuda)
    args = (inp["campos"], inp["camrotc2w"], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    whole = m.probe_rays(*args)
    m.chunk_rays = 100     # 576 rays: five full chunks and a part
    parts = m.probe_rays(*args)
    for k in PR.KEYS + ("coarse_point_opacity", "ray_mask"):
        assert torch.equal(whole[k], parts[k]), k
    got = {k: whole[k][0].cpu().numpy() for k in PR.KEYS}
    _check(got, oi, whole["coarse_point_opacity"][0].cpu().numpy(), "probe_rays")
    bare = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]))
    mb = NeuralPointsRayMarching(sc["opt"], bare, PointAggregator(sc["opt"]).to(cuda).eval())
    op = whole["coarse_point_opacity"][0]
    maps = mb.probe_maps(inp["campos"], inp["camrotc2w"], inp["raydir"][0], 2.0, 6.0, op)
    assert maps["shading_avg_color"] is None and maps["shading_avg_dir"] is None and maps["shading_avg_conf"] is None
    g = dict(oi["g"], sampled_color=None, sampled_dir=None, sampled_conf=None)
    oi_bare = dict(oi, g=g, confc=np.ones_like(oi["confc"]))
    _check({k: None if maps[k] is None else maps[k][0].cpu().numpy() for k in PR.KEYS}, oi_bare, op.cpu().numpy(),
           "no tables")


def test_probe_hole_grows_points_end_to_end(cuda):
    """A hole in the cloud -> probe_hole finds the rays around it -> grow_points
    adds their most opaque sample locations -> the next render runs on the rebuilt
    grid.  The ball holds every point the ray of pixel (8, 9) sees (CPU oracle:
    23 points removed, that one ray lost, 8 of its neighbours above 0.6, the
    nearest 0.04 from the threshold)."""
    from pointnerf_amd.checkpoint import grow_points
    from pointnerf_amd.probe import probe_hole, select_grow_candidates
    sc, _ = _ref("lego")
    H = W = 24
    params = _boosted_params()
    inp = _inputs(sc, cuda)
    with torch.no_grad():
        gt = _model(sc, cuda, params)(**inp)["coarse_raycolor"][0]
    keep = np.linalg.norm(sc["xyz"] - np.array([0.324, -0.0304, 0.5396], np.float32), axis=1) > 0.055
    assert 0 < (~keep).sum() < 100
    holed = dict(sc, **{k: np.ascontiguousarray(sc[k][keep]) for k in ("xyz", "emb", "color", "dir", "conf")})
    m = _model(holed, cuda, params)
    frame = dict(campos=inp["campos"], camrotc2w=inp["camrotc2w"], raydir=inp["raydir"][0], gt_image=gt,
                 bg_color=inp["bg_color"], pixel_idx=None, h=H, w=W)
    opt = sc["opt"]
    add = probe_hole(m, [frame], opt, opacity_thresh=0.6)
    assert opt.prob == 0 and list(opt.query_size) == [3, 3, 3]
    n_add = add[0].shape[0]
    assert n_add > 0
    # the restatement's maps of the holed cloud on the module's own opacity
    oi = PR.oracle_inputs(opt, oracle_points(holed), params, sc["campos"], sc["camrot"], sc["raydir"], sc["bg"])
    out = m.probe_rays(inp["campos"], inp["camrotc2w"], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    op = out["coarse_point_opacity"][0].cpu().numpy()
    got = {k: out[k][0].cpu().numpy() for k in PR.KEYS}
    r64 = _check(got, oi, op, "holed")
    ref_maps = dict(ray_mask=torch.from_numpy(oi["q"]["ray_mask"].astype(np.float32)).reshape(H, W, 1),
                    ray_max_shading_opacity=torch.from_numpy(r64["ray_max_shading_opacity"]).reshape(H, W, 1))
    sel = select_grow_candidates(ref_maps, gt.cpu().reshape(H, W, -1), inp["bg_color"].cpu(), None, -1.0, 0.6)
    assert int(sel.sum()) == n_add
    loc = torch.from_numpy(r64["ray_max_sample_loc_w"]).reshape(H, W, 3)[sel]
    assert torch.equal(add[0].cpu(), loc)            # every add_xyz is a selected pixel's sample location
    conf = torch.from_numpy(got["shading_avg_conf"]).reshape(H, W, 1)[sel]
    assert torch.equal(add[4].cpu(), conf * opt.prob_mul)
    n0 = m.neural_points.xyz.shape[0]
    grow_points(m.neural_points, *add)
    assert m.neural_points.xyz.shape[0] == n0 + n_add
    assert m.neural_points.points_embeding.shape[1] == n0 + n_add
    with torch.no_grad():
        again = m(**inp)
    torch.cuda.synchronize()
    assert torch.isfinite(again["coarse_raycolor"]).all()
    # the new points sit where rays sample: the grown cloud keeps every hit ray
    assert (again["ray_mask"][0].cpu().numpy() >= oi["q"]["ray_mask"]).all()
