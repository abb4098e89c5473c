"""The fused perspective frame (wcoord_query 0) on the device:
pnr_pquery_build + pnr_pquery_bufs against pnr_pquery's own rows and the CPU
restatement, pnr_composite_fwd_p against the fp64 reference on hand-built
buffers, and render_pixels against the chain run by hand, the seam forward,
itself in chunks and itself again.  Scenes, cases and references:
tests/pquery_frame_ref.py (checked on the CPU by test_pquery_frame_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

import composite_ref as CR
import pquery_frame_ref as FR
import pquery_ref as PR
from formula import formula_params
from oracle import oracle as O
from pquery_scene import pscene
from test_gpu_composite import Out, twice
from test_gpu_pquery import run as run_pquery
from test_gpu_pquery_render import device_pers, features, inputs

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = CR.Worst()
BUF_KEYS = ("ray_hit", "n_filled", "ray_off", "fill_rs", "slot_d", "pidx", "sample_p", "vflag", "valid_off",
            "valid_list", "ray_vcnt", "ray_row", "counts")


def L():
    from pointnerf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def scenes():
    """Each scene once, with the CPU restatement's query of its whole frame."""
    cache = {}

    def get(name):
        if name not in cache:
            sc = FR.scene(name)
            cache[name] = (sc, FR.ref_query(sc))
        return cache[name]
    return get


# ===================================================================== 1. buffers
def device_bufs(sc, cuda, pix, pers=None):
    """pnr_pquery_build + pnr_pquery_bufs on the scene -> numpy arrays by pnr_query_bufs' names, the S_filled
    rows of each per-sample one (plus sample_w / sample_dir)."""
    from pointnerf_amd import querier as Q
    from pointnerf_amd import querier_p as QP
    lib, opt = L(), sc["opt"]
    pers = sc["pers"] if pers is None else pers
    geo = QP.frustum_geometry(opt, sc["H"], sc["W"], sc["intrinsic"], F32(sc["near"]), F32(sc["far"]))
    qp = QP.pquery_params(opt, geo)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(cuda)   # noqa: E731
    pers_d, pix_d = t(pers, F32).reshape(-1, 3), t(pix, np.int32).reshape(-1, 2)
    campos, camrot = t(sc["campos"], F32), t(sc["camrot"], F32)
    N, R, SR, K = pers_d.shape[0], pix_d.shape[0], int(opt.SR), int(opt.K)
    dims = (lib.c_int32 * 3)(*[int(v) for v in geo.dims])
    build = lib.scratch("pnr_pquery_scratch_bytes", N, 0, SR, dims, device=cuda)
    stats = torch.zeros(8, dtype=torch.int32, device=cuda)
    st = lib.stream_ptr(cuda)
    lib.check(lib.lib().pnr_pquery_build(ctypes.byref(qp), lib.ptr(pers_d) if N else None, N, lib.ptr(stats),
                                         lib.ptr(build), build.numel(), st), "pnr_pquery_build")
    b = Q.QueryBuffers(R, SR, K, cuda)
    b.pidx.fill_(-7)
    b.fill_rs.fill_(-7)
    ray_hit = torch.full((max(R, 1),), 85, dtype=torch.int8, device=cuda)
    sdir = torch.full((max(R * SR, 1), 3), 1e30, device=cuda)
    lib.check(lib.lib().pnr_pquery_bufs(ctypes.byref(qp), N, lib.ptr(pix_d) if R else None, R, lib.ptr(campos),
                                        lib.ptr(camrot), ctypes.byref(b.c), lib.ptr(ray_hit), lib.ptr(sdir),
                                        lib.ptr(build), build.numel(), st), "pnr_pquery_bufs")
    torch.cuda.synchronize()
    counts = b.counts.cpu().numpy()
    S, Sv = int(counts[0]), int(counts[1])
    assert (counts[5:] == 0).all()
    # nothing is written past the filled samples
    assert (b.pidx[S * K:] == -7).all() and (b.fill_rs[S:] == -7).all() and (sdir[S:] == 1e30).all()
    n = lambda x: x.cpu().numpy()   # noqa: E731
    return dict(ray_hit=n(ray_hit[:R]), n_filled=n(b.n_filled[:R]), ray_off=n(b.ray_off), fill_rs=n(b.fill_rs[:S]),
                slot_d=n(b.slot_d[:S].view(torch.int16)).view(np.uint16), pidx=n(b.pidx[:S * K]).reshape(S, K),
                sample_p=n(b.sample_p[:S * 3]).reshape(S, 3), vflag=n(b.vflag[:S]), valid_off=n(b.valid_off[:S + 1]),
                valid_list=n(b.valid_list[:Sv]), ray_vcnt=n(b.ray_vcnt[:R]), ray_row=n(b.ray_row), counts=counts[:5],
                sample_w=n(b.sample_w[:S * 3]).reshape(S, 3), sample_dir=n(sdir[:S]),
                stats=dict(zip(lib.PQUERY_STATS, stats.tolist())))


def same_bufs(got, want, what):
    for k in BUF_KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape, f"{what} {k}: shape {g.shape} != {w.shape}"
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), f"{what} {k}"


def check_bufs(sc, cuda, pix, want_q=None, pers=None, what=""):
    """The device buffers of pix against pnr_pquery's rows on the same inputs
    (and the CPU restatement's, when given), pers2w against pquery_ref."""
    SR, K = int(sc["opt"].SR), int(sc["opt"].K)
    got = device_bufs(sc, cuda, pix, pers)
    FR.check_invariants(got, len(pix), SR, K)
    if len(pix):
        rows, _ = run_pquery(sc, cuda, pixel_idx=pix, pers=pers)
        assert np.array_equal(got["ray_hit"], rows["ray_mask"]), f"{what} ray_hit"
        same_bufs(got, FR.expected_bufs(rows["ray_mask"], rows["slot_z"], rows["sample_pidx"], rows["sample_loc"],
                                        SR, K), what + " vs pnr_pquery")
    if want_q is not None:
        same_bufs(got, FR.expected_from_query(want_q, SR, K), what + " vs the restatement")
    w, d = PR.pers2w(got["sample_p"], sc["camrot"], sc["campos"])
    np.testing.assert_allclose(got["sample_w"], w.reshape(-1, 3), atol=5e-6, rtol=0)
    np.testing.assert_allclose(got["sample_dir"], d.reshape(-1, 3), atol=5e-6, rtol=0)
    return got


@pytest.mark.parametrize("name", "ABC")
def test_buffers_whole_frame(cuda, scenes, name):
    sc, q = scenes(name)
    got = check_bufs(sc, cuda, sc["pixel_idx"], q, what=f"scene {name}")
    assert int(got["counts"][2]) == FR.SCENE_HIT[name]
    assert got["stats"]["n_bad_pixels"] == 0 and got["stats"]["n_points_in_grid"] == q["stats"]["n_points_in_grid"]
    if name == "A":
        assert int(((got["ray_hit"] != 0) & (got["ray_vcnt"] == 0)).sum()) >= 130
    if name == "B":
        assert int((got["n_filled"] > 64).sum()) == 552
    if name == "C":
        assert int((got["n_filled"] == 8).sum()) == 856


@pytest.mark.parametrize("name", "ABC")
def test_buffers_shuffled_subsets(cuda, scenes, name):
    sc, q = scenes(name)
    e = FR.expected_from_query(q, int(sc["opt"].SR), int(sc["opt"].K))
    for sub in FR.subsets():
        pix = np.concatenate([sc["pixel_idx"][sub], [[sc["W"], 0]]]).astype(np.int32)   # one pixel outside the frame
        got = check_bufs(sc, cuda, pix, what=f"scene {name} subset {len(sub)}")
        assert got["ray_hit"][-1] == 0 and got["n_filled"][-1] == 0
        assert np.array_equal(got["ray_hit"][:-1], e["ray_hit"][sub])
        assert np.array_equal(got["n_filled"][:-1], e["n_filled"][sub])
        # a ray's rows are those it has in the whole frame
        r = np.repeat(np.arange(len(pix)), got["n_filled"])
        src = e["ray_off"][sub[r]] + (np.arange(len(r)) - got["ray_off"][r])
        assert np.array_equal(got["pidx"], e["pidx"][src])
        assert np.array_equal(got["sample_p"].view(np.uint32), e["sample_p"][src].view(np.uint32))
        assert np.array_equal(got["slot_d"], e["slot_d"][src])


def test_buffers_empty_batches(cuda, scenes):
    sc, q = scenes("A")
    got = check_bufs(sc, cuda, np.zeros((0, 2), np.int32), what="R = 0")
    assert list(got["counts"]) == [0] * 5 and list(got["ray_off"]) == [0] and list(got["ray_row"]) == [0]
    got = check_bufs(sc, cuda, sc["pixel_idx"], pers=np.zeros((0, 3), F32), what="N = 0")
    assert list(got["counts"]) == [0] * 5 and not got["ray_hit"].any()
    miss = np.nonzero(q["ray_mask"] == 0)[0][:7]
    assert len(miss) == 7
    got = check_bufs(sc, cuda, sc["pixel_idx"][miss], what="7 misses")
    assert list(got["counts"]) == [0] * 5 and not got["ray_hit"].any() and not got["ray_off"].any()


def test_buffer_argument_checks(cuda, scenes):
    from pointnerf_amd import querier_p as QP
    sc, _ = scenes("A")
    lib = L()
    geo = QP.frustum_geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], F32(2.0), F32(6.0))
    fake = lib.c_void_p(0x1000)

    def bufs_rc(**over):
        qp = QP.pquery_params(sc["opt"], geo)
        for k, v in over.items():
            if isinstance(v, list):
                getattr(qp, k)[:] = v
            else:
                setattr(qp, k, v)
        qb = lib.QueryBufs(*([fake] * 14), 1 << 30)
        return lib.lib().pnr_pquery_bufs(ctypes.byref(qp), 10, fake, 4, fake, fake, ctypes.byref(qb), fake, fake, fake,
                                         0, None)   # build_bytes 0: refused at the latest by the size check

    for over, msg in ((dict(K=9), b"K=9"), (dict(K=0), b"K=0"), (dict(dims=[20, 16, 65536]), b"65535"),
                      (dict(kernel_size=[5, 5, 3]), b"wider than query_size"), (dict(NN=0), b"NN=0"),
                      (dict(), b"too small")):
        assert bufs_rc(**over) == lib.PNR_EINVAL
        assert msg in lib.lib().pnr_last_error(), (over, lib.lib().pnr_last_error())
    qp = QP.pquery_params(sc["opt"], geo)
    assert lib.lib().pnr_pquery_bufs(ctypes.byref(qp), 10, fake, 4, fake, fake, None, fake, fake, fake, 1 << 40,
                                     None) == lib.PNR_EINVAL
    assert b"null" in lib.lib().pnr_last_error()
    assert lib.lib().pnr_pquery_build(ctypes.byref(qp), fake, 10, None, fake, 1 << 40, None) == lib.PNR_EINVAL
    assert lib.lib().pnr_pquery_build(None, fake, 10, fake, fake, 1 << 40, None) == lib.PNR_EINVAL
    assert lib.lib().pnr_composite_fwd_p(None, None, None, 4, fake, 0.0, fake, fake, fake, fake, fake,
                                         None) == lib.PNR_EINVAL


# =================================================================== 2. composite
def composite_p(db, cp, feat_d, hit_d, zu, dev):
    R, SR, C = db.rays.R, db.qp.SR, cp.C

    def run():
        o = Out(dev)
        p = [o.new("ray_color", (R, C)), o.new("opacity", (R, SR)), o.new("is_bg", (R,)),
             o.new("ray_mask", (R,), torch.int8)]
        L().check(L().lib().pnr_composite_fwd_p(ctypes.byref(db.qp), ctypes.byref(db.qb), ctypes.byref(cp), R,
                                                L().ptr(hit_d), float(zu), L().ptr(feat_d), *p, L().stream_ptr(dev)),
                  "pnr_composite_fwd_p")
        return o
    return twice(run)


@pytest.mark.parametrize("SR,C,bg,unit", FR.P_CASES)
def test_composite_perspective_mode(cuda, SR, C, bg, unit):
    b, feat, bgc, hit, zs = FR.case_inputs(SR, C, bg, unit)
    h, vc, nf = hit.numpy(), b["ray_vcnt"].numpy(), b["n_filled"].numpy()
    assert ((h == 1) & (vc == 0)).any() and (SR == 1 or ((h == 0) & (nf > 0)).any())
    assert SR <= 64 or CR.upper_half_valid(b)
    db = CR.DevBufs(b, cuda)
    cp = db.cp(C, bgc.to(cuda) if bg else None, unit)
    feat_d = feat.to(cuda) if b["S_valid"] else torch.zeros((1, C + 1), device=cuda)
    params = dict(vsize_z=CR.VSIZE_Z, unit=unit, bg=bgc)
    miss = ~hit.bool()
    for zu in zs:
        what = f"composite_p SR={SR} C={C} bg={bg} unit={unit} zu={zu:.4f}"
        ref = FR.composite_reference_p(b, feat, hit, zu, params, torch.float64)
        o = composite_p(db, cp, feat_d, hit.to(cuda), zu, cuda)
        assert torch.equal(o["ray_mask"].cpu(), hit), what
        for k in ("ray_color", "opacity", "is_bg"):
            got = o[k].cpu()
            assert torch.isfinite(got).all(), f"{what} {k}"
            WORST.close(got, ref[k], f"composite_p.{k}", CR.TINY if k == "is_bg" else 0.0, what)
        # missed rays, whatever rows they hold: exactly bg (or 0), 0 and 1
        want = (bgc if bg else torch.zeros(C)).expand(int(miss.sum()), C)
        assert torch.equal(o["ray_color"].cpu()[miss], want), what
        assert (o["opacity"].cpu()[miss] == 0).all() and (o["is_bg"].cpu()[miss] == 1).all(), what
        # hit rays without a valid sample: exactly bg, 0 and 1 too, by marching
        e = torch.from_numpy((h == 1) & (vc == 0))
        assert torch.equal(o["ray_color"].cpu()[e], (bgc if bg else torch.zeros(C)).expand(int(e.sum()), C)), what
        assert (o["opacity"].cpu()[e] == 0).all() and (o["is_bg"].cpu()[e] == 1).all(), what


def test_composite_perspective_empty_batch(cuda):
    b, feat, bgc, hit, zs = FR.case_inputs(65, 3, True, 0)
    db = CR.DevBufs(b, cuda)
    cp = db.cp(3, bgc.to(cuda), 0)
    o = Out(cuda)
    p = [o.new("ray_color", (1, 3)), o.new("opacity", (1, 65)), o.new("is_bg", (1,)),
         o.new("ray_mask", (1,), torch.int8)]
    L().check(L().lib().pnr_composite_fwd_p(ctypes.byref(db.qp), ctypes.byref(db.qb), ctypes.byref(cp), 0, None, zs[0],
                                            None, *p, L().stream_ptr(cuda)), "pnr_composite_fwd_p")
    torch.cuda.synchronize()
    assert o.untouched()


# ======================================================================= 3. frame
def make_model(sc, cuda, params, precision="fp32", **kw):
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    agg = PointAggregator(sc["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                       torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]))
    return NeuralPointsRayMarching(sc["opt"], np_, agg.eval(), precision=precision, **kw)


def pixel_args(sc, inp, pix=None):
    """render_pixels' arguments for the scene (pix: rows of the frame, or None for all of it)."""
    p = inp["pixel_idx"][0] if pix is None else inp["pixel_idx"][0][torch.as_tensor(pix, device=inp["campos"].device)]
    return (inp["campos"][0], inp["camrotc2w"][0], p, sc["H"], sc["W"], inp["intrinsic"][0], 2.0, 6.0, inp["bg_color"])


PARAMS = dict(salt=0.2)
_CHAIN = {}


def chain(name, scenes, cuda):
    """The frame by hand, once per scene: PR.query on the perspective coordinates the module computes ->
    O.gather -> O.aggregate -> O.ray_dist -> O.ray_march -> fill (test_module_eval_forward_vs_chain_by_hand)."""
    if name in _CHAIN:
        return _CHAIN[name]
    sc, _ = scenes(name)
    params = formula_params(**PARAMS)
    m = make_model(sc, cuda, params)
    inp = inputs(sc, cuda)
    q = FR.ref_query(sc, pers=device_pers(m, inp))
    pts = dict(xyz=sc["xyz"], emb=sc["emb"], color=sc["color"], dir=sc["dir"], conf=sc["conf"])
    g = O.gather(pts, q["sample_pidx"], sc["campos"], sc["camrot"])
    feats, rv, _, _ = O.aggregate(params, g["sampled_color"], None, g["sampled_dir"], g["sampled_conf"],
                                  g["sampled_embedding"], g["sampled_xyz_pers"], g["sampled_xyz"], g["sample_pnt_mask"],
                                  q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"])
    vz = float(q["vsize"][2])
    rd = O.ray_dist(q["sample_loc"], rv, vz, sc["opt"].raydist_mode_unit)
    color, _, opacity, _, _, bgT = O.ray_march(rd, rv, feats, sc["bg"])
    hit = q["ray_mask"] > 0
    R = len(hit)
    want = dict(color=np.broadcast_to(sc["bg"][None], (R, 128)).copy(), opacity=np.zeros((R, sc["opt"].SR), F32),
                is_bg=np.ones(R, F32), ray_mask=q["ray_mask"], valid=np.zeros(R, bool))
    want["color"][hit], want["opacity"][hit], want["is_bg"][hit] = color, opacity, bgT.reshape(-1)
    want["valid"][hit] = rv.any(-1)
    with torch.no_grad():
        seam = m(**inp)
    want["seam"] = {k: v[0].cpu().numpy() for k, v in seam.items() if torch.is_tensor(v)}
    want["seam_keys"] = set(seam)
    _CHAIN[name] = want
    return want


def near(got, want, what):
    np.testing.assert_allclose(got, want, atol=2e-4, rtol=1e-4, err_msg=what)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "fp32h2"])
@pytest.mark.parametrize("name", "AB")
def test_frame_vs_chain_by_hand(cuda, scenes, name, precision):
    sc, _ = scenes(name)
    want = chain(name, scenes, cuda)
    m = make_model(sc, cuda, formula_params(**PARAMS), precision)
    color, opacity, is_bg, ray_mask = (t.cpu().numpy() for t in m.render_pixels(*pixel_args(sc, inputs(sc, cuda))))
    assert m.h2_fallbacks == 0
    what = f"scene {name} {precision}"
    assert ray_mask.dtype == np.int8 and np.array_equal(ray_mask, want["ray_mask"]), what
    near(color, want["color"], what + " colour")
    near(opacity, want["opacity"], what + " opacity")
    near(is_bg, want["is_bg"], what + " is_bg")
    # the seam forward of the same model
    near(color, want["seam"]["coarse_raycolor"], what + " colour vs seam")
    near(opacity, want["seam"]["coarse_point_opacity"], what + " opacity vs seam")
    near(is_bg, want["seam"]["coarse_is_background"][:, 0], what + " is_bg vs seam")
    assert np.array_equal(ray_mask, want["seam"]["ray_mask"])
    # missed rays and hit rays without any neighbour: exactly the background
    empty = (want["ray_mask"] > 0) & ~want["valid"]
    assert name != "A" or empty.sum() >= 130
    for rows in (empty, want["ray_mask"] == 0):
        assert np.array_equal(color[rows], np.broadcast_to(sc["bg"], (int(rows.sum()), 128))), what
        assert (is_bg[rows] == 1).all() and (opacity[rows] == 0).all(), what
    assert (ray_mask[empty] == 1).all()
    c = m.last_counts
    assert c["R_hit"] == FR.SCENE_HIT[name] and c["R_valid"] == int(want["valid"].sum())
    assert c["S_valid"] > 0 and c["S_filled"] >= c["S_valid"] and c["n_pairs"] >= c["S_valid"]


def test_frame_of_missing_rays_and_whole_frame_default(cuda, scenes):
    sc, q = scenes("A")
    m = make_model(sc, cuda, formula_params(**PARAMS))
    inp = inputs(sc, cuda)
    miss = np.nonzero(q["ray_mask"] == 0)[0][:7]
    color, opacity, is_bg, ray_mask = m.render_pixels(*pixel_args(sc, inp, miss))
    assert not ray_mask.any() and opacity.shape == (7, sc["opt"].SR) and not opacity.any() and (is_bg == 1).all()
    assert np.array_equal(color.cpu().numpy(), np.broadcast_to(sc["bg"], (7, 128)))
    assert m.last_counts["R_hit"] == 0 and m.last_counts["S_valid"] == 0
    a = pixel_args(sc, inp)
    whole = m.render_pixels(*a)
    default = m.render_pixels(a[0], a[1], None, *a[3:])       # pixel_idx None: the frame in row-major order
    for x, y in zip(whole, default):
        assert torch.equal(x, y)
    empty = m.render_pixels(a[0], a[1], a[2][:0], *a[3:])
    assert [tuple(t.shape) for t in empty] == [(0, 128), (0, sc["opt"].SR), (0,), (0,)]


# =========================================================== 4. chunks, repeatability
def test_chunks_repeats_and_reused_p1(cuda, scenes):
    sc, _ = scenes("A")
    params = formula_params(**PARAMS)
    inp = inputs(sc, cuda)
    sub1, sub2 = FR.subsets()
    for precision in ("fp32", "fp32h2"):
        m = make_model(sc, cuda, params, precision)
        whole = m.render_pixels(*pixel_args(sc, inp))
        counts = dict(m.last_counts)
        again = m.render_pixels(*pixel_args(sc, inp))
        for x, y in zip(whole, again):
            assert torch.equal(x, y), precision
        m.chunk_rays = 333
        chunked = m.render_pixels(*pixel_args(sc, inp))
        assert dict(m.last_counts) == counts
        assert torch.equal(chunked[3], whole[3])
        for x, y in zip(chunked[:3], whole[:3]):
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), atol=1e-6, rtol=0)
        m.chunk_rays = None
        # a second pixel batch on the first one's P1 against a model that never rendered
        m.render_pixels(*pixel_args(sc, inp, sub1))
        reused = m.render_pixels(*pixel_args(sc, inp, sub2), reuse_p1=True)
        fresh = make_model(sc, cuda, params, precision).render_pixels(*pixel_args(sc, inp, sub2))
        for x, y in zip(reused, fresh):
            assert torch.equal(x, y), precision
        for x, y in zip(reused, whole):
            assert torch.equal(x, y[torch.as_tensor(sub2, device=cuda)]), precision


# =================================================================== 5. interface
SEAM_KEYS = {"coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "coarse_mask", "queried_shading",
             "ray_mask"}


def test_forward_routes_through_render_pixels(cuda, scenes):
    from test_gpu_pquery_render import lone_point_scene
    params = formula_params(**PARAMS)
    sc = lone_point_scene(zero_one_loss_items=[])         # no loss reads the aux outputs
    inp = inputs(sc, cuda)
    default, fused = make_model(sc, cuda, params), make_model(sc, cuda, params, fused_perspective=True)
    assert not fused.wants_aux()
    with torch.no_grad():
        want, got = default(**inp), fused(**inp)
    assert fused.last_counts is not None and default.last_counts is None    # only render_pixels sets them
    assert set(got) == set(want) == SEAM_KEYS
    for k in SEAM_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    for k in ("ray_mask", "queried_shading"):
        assert torch.equal(got[k], want[k]), k
    assert (want["queried_shading"][0, :, 0] == 1).sum() > (want["ray_mask"] == 0).sum()   # neighbour-less hit rays
    for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "coarse_mask"):
        near(got[k].cpu().numpy(), want[k].cpu().numpy(), k)
    # aux wanted (the scene's default options): the seam path, unchanged
    sc, _ = scenes("A")
    inp = inputs(sc, cuda)
    default, fused = make_model(sc, cuda, params), make_model(sc, cuda, params, fused_perspective=True)
    assert fused.wants_aux()
    with torch.no_grad():
        want, got = default(**inp), fused(**inp)
    assert fused.last_counts is None
    assert set(got) == set(want) == SEAM_KEYS | {"weight", "blend_weight", "conf_coefficient"}
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_render_pixels_refusals_and_events(cuda, scenes):
    from pointnerf_amd._lib import PnrError
    params = formula_params(**PARAMS)
    sc, _ = scenes("A")
    inp = inputs(sc, cuda)
    with pytest.raises(PnrError, match="bf16"):
        make_model(sc, cuda, params, "bf16").render_pixels(*pixel_args(sc, inp))
    world = features(pscene(wcoord_query=1))
    with pytest.raises(PnrError, match="render_rays"):
        make_model(world, cuda, params).render_pixels(*pixel_args(world, inputs(world, cuda)))
    k16 = features(pscene(K=16, NN=1))
    with pytest.raises(PnrError, match="K = 16"):
        make_model(k16, cuda, params).render_pixels(*pixel_args(k16, inputs(k16, cuda)))
    wide = features(pscene())
    m = make_model(wide, cuda, params)
    wide["opt"].kernel_size = [5, 5, 3]                   # the querier's own constructor refuses it too
    with pytest.raises(PnrError, match="wider than query_size"):
        m.render_pixels(*pixel_args(wide, inputs(wide, cuda)))
    # the fused world-only paths still refuse a perspective model, now pointing here
    m = make_model(sc, cuda, params)
    with pytest.raises(PnrError, match="world-query only.*render_pixels"):
        m.render_rays(inp["campos"][0], inp["camrotc2w"][0], inp["raydir"][0], 2.0, 6.0, inp["bg_color"])
    events = []
    m.chunk_rays = 700
    m.render_pixels(*pixel_args(sc, inp), events=events)
    torch.cuda.synchronize()
    assert [e[0] for e in events] == ["build"] + ["query", "aggregate", "composite"] * 2
    assert all(a.elapsed_time(b) >= 0 for _, a, b in events)


def test_h2_range_flag_and_fallback_in_render_pixels(cuda, scenes):
    """test_gpu_x3.py::test_h2_range_flag_and_fallback on render_pixels: an activation beyond the f16
    range re-renders the call on fp32x3, bit-identical to an fp32x3 render_pixels; h2 stays off for those
    weights until they change; a caller's events hold one call's stages."""
    from pointnerf_amd.renderer import NeuralPointsRayMarching
    sc, _ = scenes("C")
    m = make_model(sc, cuda, formula_params(**PARAMS), "fp32h2")
    agg = m.aggregator
    mx = NeuralPointsRayMarching(sc["opt"], m.neural_points, agg, precision="fp32x3")
    a = pixel_args(sc, inputs(sc, cuda))
    one_call = ["build", "query", "aggregate", "composite"]
    with torch.no_grad():
        events = []
        m.render_pixels(*a, events=events)
        assert agg.h2_range_ok() and m.h2_fallbacks == 0 and [e[0] for e in events] == one_call
        agg.block1[2].bias.fill_(1e6)            # block1.2 outputs ~1e6 > 65504 (repacked: new version)
        events = [("mine", None, None)]
        got = m.render_pixels(*a, events=events, reuse_p1=True)
        assert m.h2_fallbacks == 1 and agg.h2_range_ok()   # flag consumed by the fallback
        assert [e[0] for e in events] == ["mine"] + one_call   # the fp32x3 run's, the h2 run's dropped
        want = mx.render_pixels(*a)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert got[3].any()
        again = m.render_pixels(*a)              # blocked weights: straight to fp32x3
        assert m.h2_fallbacks == 1 and agg.h2_range_ok()
        for x, y in zip(again, want):
            assert torch.equal(x, y)
        agg.block1[2].bias.fill_(0.0)            # new weights: h2 again, no trip
        m.render_pixels(*a)
        assert m.h2_fallbacks == 1 and m._h2_blocked_key is None and agg.h2_range_ok()
