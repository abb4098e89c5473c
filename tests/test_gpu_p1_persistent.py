"""P1 (block1.0's per-point half) as prepared model state.

The render state keeps P1 in a table of its own, valid while the key it was
built from -- precision, point count, storage and version of the embedding and
of block1.0 -- is the call's; `_RenderState.p1_builds` counts the builds.  Every
render here is compared bit for bit with the render of a model that has never
rendered before (its P1 is built by that very call).

The native half: the pnr_aggregate_fwd*_p1 calls take P1 outside the scratch, whose layout
is then that of a call without points.  (A zero row in the table for the empty
neighbour slots, with a render kernel that parks the rows as loaded, was
measured and not kept: DESIGN §36.)  Direct calls at the sizes of
tests/test_gpu_h2_producers.py (5 / 2061 / 8323 samples, K = 8 and the K = 5
build), with samples of 0, 1 and K - 1 neighbours and, from 2061 samples on,
one 8-sample tile whose 64 slots are all empty (samples 8..15): the render
kernel on the table against the general kernel (PNR_H2_GENERAL, P1 at the head
of the scratch) bit for bit and against the float64 oracle inside the bound
that file states:
  max |h2 - ref64| <= 2 max |ref32 - ref64| + 1e-7 max|ref64|
  rms              <= 1.5 rms(ref32 - ref64) + 1e-8 max|ref64|
The oracle treats every sample on its own, so the references of the samples
left as they were are test_gpu_h2_windows' own rows; only the 5-sample case,
whose neighbour lists are edited, is run through the oracle again."""
import functools

import numpy as np
import pytest
import torch

from formula import formula_params
from scenes import scene
from test_gpu_h2_acc2 import K, N_POINTS
from test_gpu_h2_producers import K5, _oracle_pair, _refs_k5, _run, _same
from test_gpu_h2_windows import COUNTS, _bound, _hid_oracle, _refs

pytestmark = pytest.mark.gpu

N_PTS, HW = 20000, 40
OUT = ("ray_color", "opacity", "is_bg", "ray_mask")


# ------------------------------------------------------------------ render calls
@functools.lru_cache(maxsize=None)
def _scene(theta, n=N_PTS):
    return scene(n, H=HW, W=HW, theta=theta)


def _model(cuda, precision="fp32h2", n=N_PTS, chunk=None, mutate=None):
    """A model over the first n points of the scene that has rendered nothing yet."""
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    sc = _scene(30.0)
    agg = PointAggregator(sc["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in formula_params(salt=0.4).items()})
    np_ = NeuralPoints(sc["opt"], cuda, *(torch.from_numpy(sc[k][:n]) for k in ("xyz", "emb", "color", "dir", "conf")))
    m = NeuralPointsRayMarching(sc["opt"], np_, agg.eval(), chunk_rays=chunk, precision=precision)
    if mutate is not None:
        with torch.no_grad():
            mutate(m)
    return m


def _cam(cuda, theta):
    sc = _scene(theta)
    return tuple(torch.from_numpy(sc[k]).to(cuda) for k in ("campos", "camrot", "raydir"))


def _bg(cuda):
    return torch.from_numpy(_scene(30.0)["bg"]).to(cuda)


def _render(m, cuda, theta, **kw):
    out = [t.clone() for t in m.render_rays(*_cam(cuda, theta), 2.0, 6.0, _bg(cuda), **kw)]
    assert int(out[3].sum()) > 100   # the camera sees the cloud
    return out


def _equal(a, b):
    for name, x, y in zip(OUT, a, b):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("per_frame", [False, True])
def test_second_camera_reuses_p1(cuda, monkeypatch, per_frame):
    """Two cameras on one model: the second call builds no P1 and renders what a fresh model renders;
    with PNR_P1_PER_FRAME=1 every call builds it, with the same outputs."""
    if per_frame:
        monkeypatch.setenv("PNR_P1_PER_FRAME", "1")
    m = _model(cuda)
    _render(m, cuda, 30.0)
    assert m._state.p1_builds == 1
    got = _render(m, cuda, 200.0)
    assert m._state.p1_builds == (2 if per_frame else 1)
    _equal(got, _render(_model(cuda), cuda, 200.0))
    _render(m, cuda, 30.0, reuse_p1=True)   # the hint: no build either way
    assert m._state.p1_builds == (2 if per_frame else 1)


def _edit_emb(m):
    m.neural_points.points_embeding.mul_(1.25)


def _edit_weight(m):
    m.aggregator.block1[0].weight.mul_(0.5)


def _edit_bias(m):
    m.aggregator.block1[0].bias.add_(0.125)


def _sgd_step(m):
    ps = [m.neural_points.points_embeding, m.aggregator.block1[0].weight, m.aggregator.block1[0].bias]
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    torch.optim.SGD(ps, lr=0.0625).step()
    for p in ps:
        p.grad = None


@pytest.mark.parametrize("edit", [_edit_emb, _edit_weight, _edit_bias, _sgd_step], ids=lambda f: f.__name__.strip("_"))
def test_in_place_change_rebuilds_p1_once(cuda, edit):
    m = _model(cuda)
    before = _render(m, cuda, 200.0)
    with torch.no_grad():
        edit(m)
    got = _render(m, cuda, 200.0)
    assert m._state.p1_builds == 2
    _equal(got, _render(_model(cuda, mutate=edit), cuda, 200.0))
    assert not torch.equal(got[0], before[0])
    _equal(_render(m, cuda, 200.0), got)
    assert m._state.p1_builds == 2


def test_new_point_count_rebuilds_p1_once(cuda):
    m = _model(cuda)
    _render(m, cuda, 200.0)
    small = _model(cuda, n=15000)
    m.neural_points = small.neural_points
    got = _render(m, cuda, 200.0)
    assert m._state.p1_builds == 2 and m._state.p1.shape[0] == 15000
    _equal(got, _render(_model(cuda, n=15000), cuda, 200.0))
    _render(m, cuda, 30.0)
    assert m._state.p1_builds == 2


def test_precision_change_rebuilds_p1(cuda):
    """fp32h2 (k_point_pre_h2), fp32x3 (the fp32 k_point_pre), fp32h2 again: one table, never mistaken."""
    m = _model(cuda)
    want = {p: _render(_model(cuda, precision=p), cuda, 200.0) for p in ("fp32h2", "fp32x3")}
    for i, p in enumerate(("fp32h2", "fp32x3", "fp32h2")):
        m.precision = p
        _equal(_render(m, cuda, 200.0), want[p])
        assert m._state.p1_builds == i + 1


def test_range_fallback_keeps_the_tables_apart(cuda):
    """A block1.2 bias of 1e6 trips the range flag: the call is rendered again on fp32x3, whose P1 replaces
    the h2 one in the table; with the bias restored the h2 P1 is built again."""
    def trip(m):
        m.aggregator.block1[2].bias.fill_(1e6)

    m = _model(cuda)
    clean = _render(m, cuda, 200.0)
    bias = m.aggregator.block1[2].bias.detach().clone()
    with torch.no_grad():
        trip(m)
    got = m.render_rays(*_cam(cuda, 200.0), 2.0, 6.0, _bg(cuda))
    assert m.h2_fallbacks == 1 and m._state.p1_builds == 2   # P1 itself is in range: the h2 one stood, the x3 one is new
    want = _model(cuda, precision="fp32x3", mutate=trip).render_rays(*_cam(cuda, 200.0), 2.0, 6.0, _bg(cuda))
    _equal(got, want)
    with torch.no_grad():
        m.aggregator.block1[2].bias.copy_(bias)
    _equal(_render(m, cuda, 200.0), clean)
    _equal(clean, _render(_model(cuda), cuda, 200.0))
    assert m.h2_fallbacks == 1 and m._state.p1_builds == 3


def test_scratch_growth_keeps_p1(cuda):
    m = _model(cuda)
    cp, cr, rd = _cam(cuda, 200.0)
    m.render_rays(cp, cr, rd[:160].contiguous(), 2.0, 6.0, _bg(cuda))
    small, rows = m.last_counts["S_valid"], m._state.scratch_rows
    got = _render(m, cuda, 200.0)
    assert m.last_counts["S_valid"] > 1.5 * max(small, 1) and m._state.scratch_rows > rows   # the scratch grew
    assert m._state.p1_builds == 1
    _equal(got, _render(_model(cuda), cuda, 200.0))


def test_call_without_samples_leaves_p1_unbuilt(cuda):
    """A first call whose rays miss the cloud launches no aggregate kernel, so it must not mark P1 built."""
    m = _model(cuda)
    cp, cr, rd = _cam(cuda, 200.0)
    out = m.render_rays(cp, cr, (-rd).contiguous(), 2.0, 6.0, _bg(cuda))
    assert int(out[3].sum()) == 0 and m.last_counts["S_valid"] == 0 and m._state.p1_builds == 0
    _equal(_render(m, cuda, 200.0), _render(_model(cuda), cuda, 200.0))
    assert m._state.p1_builds == 1


def test_chunked_call_builds_p1_once(cuda):
    m = _model(cuda, chunk=333)   # five chunks, the last one partial
    a = _render(m, cuda, 200.0)
    b = _render(m, cuda, 30.0)
    assert m._state.p1_builds == 1
    fresh = _model(cuda, chunk=333)
    _equal(b, _render(fresh, cuda, 30.0))
    _equal(a, _render(fresh, cuda, 200.0))


def test_queued_calls_build_p1_once_on_the_side_stream(cuda):
    """sync=False calls: the first one builds P1 on the side stream, the next ones build none; every call
    keeps its "p1" stage line, which is empty where nothing was built."""
    m = _model(cuda)
    m.p1_side_max_points_per_ray = 1e9   # the test scene has more points than rays
    _render(m, cuda, 30.0)               # the first call runs synchronously and sizes the queue
    with torch.no_grad():
        m.neural_points.points_embeding.add_(0.0)   # same values, new version
    evs = [[], [], []]
    got = [m.render_rays(*_cam(cuda, th), 2.0, 6.0, _bg(cuda), sync=False, events=ev)
           for th, ev in zip((200.0, 30.0, 200.0), evs)]
    m.finish()
    assert [[e[0] for e in ev].count("p1") for ev in evs] == [1, 1, 1] and m._state.p1_builds == 2
    torch.cuda.synchronize()
    ms = [[a.elapsed_time(b) for name, a, b in ev if name == "p1"][0] for ev in evs]
    print("p1 stage ms per call:", ms)
    assert ms[1] < ms[0] and ms[2] < ms[0]   # two event records back to back against a kernel over 20000 points
    fresh = _model(cuda)
    for th, g in zip((200.0, 30.0, 200.0), got):
        _equal(g, _render(fresh, cuda, th))


def test_camera_batch_builds_p1_once(cuda):
    m = _model(cuda)
    views = [_cam(cuda, 30.0), _cam(cuda, 200.0)]
    a = m.render_views(views, 2.0, 6.0, _bg(cuda))
    b = m.render_views(views[::-1], 2.0, 6.0, _bg(cuda))
    assert m._state.p1_builds == 1
    for x, y in zip(a, b[::-1]):
        _equal(x, y)
    _equal(_model(cuda).render_views(views[::-1], 2.0, 6.0, _bg(cuda))[0], b[0])


def test_captured_graph_keeps_p1_in_the_graph(cuda):
    """RenderGraph: the sizing render builds P1 into the graph's own table, the warm-up takes it, and the
    captured run holds a build of its own, so a replay never depends on what the host believed valid."""
    from pointnerf_amd.renderer import RenderGraph
    m = _model(cuda)
    want = _render(m, cuda, 200.0)
    g = RenderGraph(m, *_cam(cuda, 200.0), 2.0, 6.0, _bg(cuda), margin=3.0)   # room for the other camera's samples
    assert g.state.p1_builds == 2 and m._state.p1_builds == 1
    out = g.replay()
    assert g.check()
    _equal(out, want)
    out = g.replay(*_cam(cuda, 30.0))
    assert g.check() and g.state.p1_builds == 2
    _equal(out, _render(m, cuda, 30.0))


# ------------------------------------------------- empty slots on the table, direct
@functools.lru_cache(maxsize=None)
def _zero_case(n, k):
    """(case, hid32, hid64) with an all-empty tile and samples of 0, 1 and k - 1 neighbours."""
    cs, h32, h64 = _refs(n) if k == K else _refs_k5(n)
    pidx = np.array(cs["pidx"])
    if n < 16:   # 5 samples: neighbour counts k, 1, k - 1, 0, as it was -- through the oracle again
        pidx[1, 1:] = -1
        pidx[2, :k - 1] = (37 * np.arange(k - 1) + 11) % N_POINTS
        pidx[2, k - 1:] = -1
        ref32, ref64, rv = _oracle_pair(cs, pidx, cs["campos"], cs["camrot"], cs["loc_p"])
        c = dict(cs, pidx=pidx, ref32=ref32, ref64=ref64, rv=rv)
        h32, a32 = _hid_oracle(c, False)
        h64, a64 = _hid_oracle(c, True)
        assert np.array_equal(a32, ref32[rv, 0]) and np.array_equal(a64, ref64[rv, 0])
    else:        # samples 8..15 (one tile, 64 slots) emptied; every other sample keeps its reference rows
        pidx[8:16] = -1
        rows = np.flatnonzero(cs["rv"])
        keep = (rows < 8) | (rows >= 16)
        rv = np.array(cs["rv"])
        rv[8:16] = False
        c = dict(cs, pidx=pidx, rv=rv)
        h32, h64 = h32[keep], h64[keep]
    cnt = (c["pidx"][:, :k] >= 0).sum(1)
    assert {0, 1, k - 1, k} <= set(cnt.tolist()) and np.array_equal(cnt > 0, c["rv"])
    return c, h32, h64


def _run_table(cs, cuda, k):
    """pnr_aggregate_fwd_h2 as the frame render calls it, P1 in a table of its own -> the dict of
    test_gpu_h2_producers._run."""
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints
    pt = cs["points"]
    agg = PointAggregator(cs["opt"]).to(cuda)
    agg.load_state_dict({k_: torch.from_numpy(v) for k_, v in cs["params"].items()})
    agg.eval()
    np_ = NeuralPoints(cs["opt"], cuda, *(torch.from_numpy(np.array(pt[k_])) for k_ in ("xyz", "emb", "color", "dir", "conf")))
    n = cs["pidx"].shape[0]
    host = dict(campos=cs["campos"], camrot=cs["camrot"], pidx=cs["pidx"][:, :k], loc_w=cs["loc_w"], loc_p=cs["loc_p"],
                vd=cs["vd"])
    dev = {k_: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k_, v in host.items()}
    ident = torch.arange(n, dtype=torch.int32, device=cuda)
    s = L.Samples(None, None, n, dev["pidx"].data_ptr(), dev["loc_w"].data_ptr(), dev["loc_p"].data_ptr(),
                  dev["vd"].data_ptr(), ident.data_ptr(), 1, k, None)
    pts, _keep = np_.tables(dev["campos"], dev["camrot"])
    table = torch.full((int(pts.n) + 1, 256), float("nan"), device=cuda)   # one guard row behind the table
    mlp, _k1 = agg.packed()
    mlph, _k2 = agg.packed_h2()
    nm = -(-n // 64) * 64
    h0 = 256   # scratch = one unused row | hid planes [tiles of 64 samples] | vmask
    f = torch.zeros((n, 129), device=cuda)
    scr = L.aggregate_scratch(n, 0, cuda).zero_()
    L.check(L.lib().pnr_aggregate_fwd_h2_p1(L.ctypes.byref(pts), L.ctypes.byref(s), L.ctypes.byref(mlp),
                                            L.ctypes.byref(mlph), L.ptr(table), L.ptr(f), None, None, L.ptr(scr),
                                            scr.numel() * 4, L.stream_ptr(cuda)), "pnr_aggregate_fwd_h2_p1")
    torch.cuda.synchronize()
    assert agg.h2_range_ok()
    # P1 went into the table (every row, none behind it) and not into the scratch's unused row
    assert bool(torch.isfinite(table[:-1]).all()) and bool(torch.isnan(table[-1]).all()) and not scr[:h0].any()
    raw = scr[h0:h0 + nm * 256].cpu().numpy().view(np.float16).reshape(nm // 64, 2, 32, 64, 8)
    bits = np.ascontiguousarray(raw.view(np.uint16).transpose(0, 3, 1, 2, 4)).reshape(nm, 2, 256)[:n]
    x = raw[:, 0].astype(np.float64) + raw[:, 1].astype(np.float64) / 2048.0
    hid = x.transpose(0, 2, 1, 3).reshape(nm, 256)[:n]
    vmask = scr[h0 + nm * 256:h0 + nm * 256 + n].view(torch.int32).cpu().numpy()
    return dict(out=f.cpu().numpy(), bits=bits, hid=hid, vmask=vmask)


@pytest.mark.parametrize("k", [K, K5])
@pytest.mark.parametrize("n", COUNTS)
def test_empty_slots_on_the_table_equal_general_and_oracle_bound(cuda, n, k):
    cs, h32, h64 = _zero_case(n, k)
    rv = cs["rv"]
    general = _run(cs, cuda, k=k, general=True)[0][0]
    r = _run_table(cs, cuda, k)
    _same(r, general, rv)
    assert np.array_equal(r["vmask"] != 0, rv)
    assert not r["out"][~rv].any() and not r["hid"][~rv].any()   # samples without a neighbour stay unwritten
    if n >= 16:
        assert not rv[8:16].any() and rv[:8].any() and rv[16:24].any()   # the empty tile between two live ones
    ref32, ref64 = cs["ref32"], cs["ref64"]   # (rows 8..15 of the larger cases are stale and not read: ~rv)
    _bound(r["hid"][rv], h32, h64, f"hid table n={n} K={k}")
    _bound(r["out"][rv, 0], ref32[rv, 0], ref64[rv, 0], f"alpha table n={n} K={k}")
    _bound(r["out"][rv], ref32[rv], ref64[rv], f"features table n={n} K={k}")
