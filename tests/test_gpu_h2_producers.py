"""k_pairs_h2's render specialisation k_pairs_h2_rs (aggregate_x3.hip): launch
constants from an LDS block, the P1 row ids read wide, the launch-fixed options
resolved when the kernel is picked.  Same arithmetic, so the outputs must be the
general kernel's bit for bit.

The launch code picks k_pairs_h2_rs when the call has no `pers` table, no
`used_map`, no per-point `rw2c`, colour / dir / conf tables, a `dir_map`, one
camera and no `out_weight` / `out_conf` (the frame render's call; its `dir_map`
is always there, so here it is the ABSENT `dir_map` that disqualifies), and the
general k_pairs_h2 otherwise or when PNR_H2_GENERAL is set.  The base call of
this file is the case of tests/test_gpu_h2_windows.py (3001 points, 1..8
neighbours per sample with -1 slots behind them, one sample with none) with an
identity `dir_map`; every disqualifying option is set to a neutral value in
turn.

Sizes (those of test_gpu_h2_windows.py): 5 samples (less than one tile, lanes
past eff_n), 2061 (258 tiles: every workgroup's first tile and a few second
ones -- a hoisted value right only on the first iteration), 8323 (1041 tiles:
several loop iterations per workgroup, the XCD hand-out).  None is a multiple of
8: the last tile is not full.  Each size also as a second build with K = 5
(pidx [n, 5]), whose reference is the K = 8 case with slots 5..7 emptied.

Bound (the one test_gpu_h2_windows.py states), against the float64 oracle with
the float32 oracle's own error as the yardstick, for hid (put together from its
planes), alpha and the features:
  max |h2 - ref64| <= 2 max |ref32 - ref64| + 1e-7 max|ref64|
  rms              <= 1.5 rms(ref32 - ref64) + 1e-8 max|ref64|"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_h2_acc2 import K, _oracle_f64
from test_gpu_h2_windows import COUNTS, _bound, _hid_oracle, _refs

pytestmark = pytest.mark.gpu
K5 = 5


def _oracle_pair(cs, pidx, campos, camrot, loc_p, rw=None):
    """(ref32, ref64, rv) of oracle.aggregate, as test_gpu_h2_acc2._case runs it."""
    points = dict(cs["points"])
    if rw is not None:
        points["Rw2c"] = rw
    g = O.gather(points, pidx[:, None, :], campos, camrot)

    def run(prm):
        out, rv, _, _ = O.aggregate(prm, g["sampled_color"], g["sampled_Rw2c"], g["sampled_dir"], g["sampled_conf"],
                                    g["sampled_embedding"], g["sampled_xyz_pers"], g["sampled_xyz"],
                                    g["sample_pnt_mask"], loc_p[:, None, :], cs["loc_w"][:, None, :], cs["vd"][:, None, :])
        return np.asarray(out)[:, 0], np.asarray(rv)[:, 0]

    ref32, rv = run(cs["params"])
    with _oracle_f64():
        ref64, _ = run({k: v.astype(np.float64) for k, v in cs["params"].items()})
    assert ref32.dtype == np.float32 and ref64.dtype == np.float64
    return ref32, ref64, rv


@functools.lru_cache(maxsize=None)
def _refs_k5(n):
    """The K = 5 build: the case with slots 5..7 emptied, its oracle results and hid references."""
    cs = _refs(n)[0]
    pidx = np.array(cs["pidx"])
    pidx[:, K5:] = -1
    ref32, ref64, rv = _oracle_pair(cs, pidx, cs["campos"], cs["camrot"], cs["loc_p"])
    c5 = dict(cs, pidx=pidx, ref32=ref32, ref64=ref64, rv=rv)
    h32, a32 = _hid_oracle(c5, False)
    h64, a64 = _hid_oracle(c5, True)
    assert np.array_equal(a32, ref32[rv, 0]) and np.array_equal(a64, ref64[rv, 0])
    for a in (pidx, ref32, ref64, h32, h64):
        a.setflags(write=False)
    return c5, h32, h64


def _rotations(n, seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return np.ascontiguousarray(q.astype(np.float32))


def _fma32(a, b, c):
    """float32 fma(a, b, c), one rounding: the float64 product is exact, its sum
    with c is rounded to odd in float64 (TwoSum gives the exact error), and 53
    bits rounded to odd then round to 24 bits as the exact value does."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _pers_table(xyz, campos, camrot):
    """What pair_pers leaves in pp: world_to_pers (pnr_common.h) as aggregate_x3.hip
    compiles it, with the sum (s0 R0j + s1 R1j) + s2 R2j of s = p - c contracted
    into fma(s2, R2j, fma(s0, R0j, s1 R1j)) (the gather's sum102), then
    (x0 / x2, x1 / x2, x2) with correctly rounded divisions."""
    f = np.float32
    s = (xyz.astype(f) - campos.astype(f)[None, :]).astype(f)
    R = camrot.astype(f)
    x = [_fma32(s[:, 2], R[2, j], _fma32(s[:, 0], R[0, j], (s[:, 1] * R[1, j]).astype(f))) for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.stack([(x[0] / x[2]).astype(f), (x[1] / x[2]).astype(f), x[2]], 1))


@contextlib.contextmanager
def _force_general(on):
    old = os.environ.get("PNR_H2_GENERAL")
    if on:
        os.environ["PNR_H2_GENERAL"] = "1"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["PNR_H2_GENERAL"]
            else:
                os.environ["PNR_H2_GENERAL"] = old


def _run(cs, cuda, *, k=K, dir_map=True, pers=False, used=False, want_wc=False, rw=None, cams=None, general=False,
         launches=1, mutate=None, check_range=True, roll=0):
    """pnr_aggregate_fwd_h2 on zeroed scratch -> per launch (out [n, 129], hid bits
    [n, 2, 256] uint16 (hi, lo planes per sample), hid [n, 256] float64, vmask [n]); the aggregator.
    roll: the sample list rotated by that many samples (outputs come back un-rotated).
    cams: (campos [C, 3], camrot [C, 3, 3], ray_cam [n], loc_p [n, 3]) for a camera batch."""
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints
    pt = cs["points"]
    agg = PointAggregator(cs["opt"]).to(cuda)
    agg.load_state_dict({k_: torch.from_numpy(v) for k_, v in cs["params"].items()})
    agg.eval()
    if mutate is not None:
        with torch.no_grad():
            mutate(agg)
    np_ = NeuralPoints(cs["opt"], cuda, *(torch.from_numpy(np.array(pt[k_])) for k_ in ("xyz", "emb", "color", "dir", "conf")))
    n = cs["pidx"].shape[0]
    rl = (lambda a: np.roll(a, roll, axis=0)) if roll else (lambda a: a)
    host = dict(campos=cs["campos"], camrot=cs["camrot"], pidx=rl(cs["pidx"][:, :k]), loc_w=rl(cs["loc_w"]),
                loc_p=rl(cs["loc_p"]), vd=rl(cs["vd"]))
    ray_cam = None
    if cams is not None:
        host.update(campos=cams[0], camrot=cams[1], loc_p=rl(cams[3]))
        ray_cam = torch.from_numpy(np.ascontiguousarray(rl(cams[2]).astype(np.int32))).to(cuda)
    dev = {k_: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k_, v in host.items()}
    ident = torch.arange(max(n, int(pt["xyz"].shape[0])), dtype=torch.int32, device=cuda)
    s = L.Samples(None, None, n, dev["pidx"].data_ptr(), dev["loc_w"].data_ptr(), dev["loc_p"].data_ptr(),
                  dev["vd"].data_ptr(), ident.data_ptr() if dir_map else None, 1, k, L.ptr(ray_cam))
    pts, _keep = np_.tables(dev["campos"], dev["camrot"])
    keep = []
    if pers:
        keep.append(torch.from_numpy(_pers_table(np.array(pt["xyz"]), cs["campos"], cs["camrot"])).to(cuda))
        pts.pers = keep[-1].data_ptr()
    if used:   # every point used, in order: P1 row = point row
        pts.used, pts.n_used, pts.used_map = ident.data_ptr(), int(pts.n), ident.data_ptr()
    if rw is not None:
        keep.append(torch.from_numpy(rw.reshape(-1, 9)).to(cuda).contiguous())
        pts.rw2c = keep[-1].data_ptr()
    mlp, _k1 = agg.packed()
    mlph, _k2 = agg.packed_h2()
    nm = -(-n // 64) * 64
    h0 = int(pts.n) * 256   # scratch = P1 [points, 256] | hid planes [tiles of 64 samples] | vmask
    outs = []
    with _force_general(general):
        for _ in range(launches):
            f = torch.zeros((n, 129), device=cuda)
            wc = [torch.full((n, k), -7.0, device=cuda) for _ in range(2)] if want_wc else [None, None]
            scr = L.aggregate_scratch(n, pts.n, cuda).zero_()
            L.check(L.lib().pnr_aggregate_fwd_h2(L.ctypes.byref(pts), L.ctypes.byref(s), L.ctypes.byref(mlp),
                                                 L.ctypes.byref(mlph), L.ptr(f), L.ptr(wc[0]), L.ptr(wc[1]), L.ptr(scr),
                                                 scr.numel() * 4, L.stream_ptr(cuda)), "pnr_aggregate_fwd_h2")
            outs.append((f, scr, wc))
        torch.cuda.synchronize()
    if check_range:
        assert agg.h2_range_ok()
    un = (lambda a: np.roll(a, -roll, axis=0)) if roll else (lambda a: a)
    res = []
    for f, scr, wc in outs:
        raw = scr[h0:h0 + nm * 256].cpu().numpy().view(np.float16).reshape(nm // 64, 2, 32, 64, 8)
        bits = np.ascontiguousarray(raw.view(np.uint16).transpose(0, 3, 1, 2, 4)).reshape(nm, 2, 256)[:n]
        with np.errstate(invalid="ignore"):   # (the range-flag case holds inf halves)
            x = raw[:, 0].astype(np.float64) + raw[:, 1].astype(np.float64) / 2048.0
        hid = x.transpose(0, 2, 1, 3).reshape(nm, 256)[:n]
        vmask = scr[h0 + nm * 256:h0 + nm * 256 + n].view(torch.int32).cpu().numpy()
        r = dict(out=un(f.cpu().numpy()), bits=un(bits), hid=un(hid), vmask=un(vmask))
        if want_wc:
            r["w"], r["c"] = un(wc[0].cpu().numpy()), un(wc[1].cpu().numpy())
        res.append(r)
    return res, agg


def _same(a, b, rv):
    """Bit-identical outputs; hid planes on the samples with a neighbour (the others are never written)."""
    assert np.array_equal(a["out"].view(np.uint32), b["out"].view(np.uint32))
    assert np.array_equal(a["vmask"], b["vmask"])
    assert np.array_equal(a["bits"][rv], b["bits"][rv])


@functools.lru_cache(maxsize=None)
def _base(cuda, n, k):
    """The specialised route's result of the base call (computed once, read-only)."""
    cs = _refs(n)[0] if k == K else _refs_k5(n)[0]
    r = _run(cs, cuda, k=k)[0][0]
    for a in r.values():
        a.setflags(write=False)
    return r


@pytest.mark.parametrize("k", [K, K5])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("route", ["specialised", "general"])
def test_h2_producers_oracle_bound(cuda, route, n, k):
    cs, h32, h64 = _refs(n) if k == K else _refs_k5(n)
    r = _base(cuda, n, k) if route == "specialised" else _run(cs, cuda, k=k, general=True)[0][0]
    rv = cs["rv"]
    assert np.array_equal(r["vmask"] != 0, rv)
    assert not r["out"][~rv].any() and not r["hid"][~rv].any()   # samples without a neighbour stay unwritten
    _bound(r["hid"][rv], h32, h64, f"hid {route} n={n} K={k}")
    _bound(r["out"][:, 0], cs["ref32"][:, 0], cs["ref64"][:, 0], f"alpha {route} n={n} K={k}")
    _bound(r["out"], cs["ref32"], cs["ref64"], f"features {route} n={n} K={k}")


@pytest.mark.parametrize("k", [K, K5])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("option", ["forced", "no_dir_map", "pers", "used_map", "out_weight_conf"])
def test_h2_producers_route_equality(cuda, option, n, k):
    """The general kernel, reached by each disqualifying option at a neutral value
    (and by PNR_H2_GENERAL on the very same call), against the specialised one."""
    cs = _refs(n)[0] if k == K else _refs_k5(n)[0]
    kw = dict(forced=dict(general=True), no_dir_map=dict(dir_map=False), pers=dict(pers=True), used_map=dict(used=True),
              out_weight_conf=dict(want_wc=True))[option]
    r = _run(cs, cuda, k=k, **kw)[0][0]
    _same(r, _base(cuda, n, k), cs["rv"])
    if option == "out_weight_conf":   # written for every slot k < K of every sample, normalised weights
        assert (r["w"] >= 0).all() and (r["c"] > 0).all()
        np.testing.assert_allclose(r["w"].sum(1)[cs["rv"]], 1.0, atol=1e-5)


def test_h2_producers_k5_is_masked_k8(cuda):
    """pidx [n, 5] and pidx [n, 8] with slots 5..7 empty are the same samples."""
    for n in COUNTS:
        c5 = _refs_k5(n)[0]
        _same(_run(c5, cuda, k=K)[0][0], _base(cuda, n, K5), c5["rv"])


@pytest.mark.parametrize("n", COUNTS)
def test_h2_producers_point_rw2c_vs_oracle(cuda, n):
    """A per-point Rw2c table changes the arithmetic: the general kernel, against the oracle."""
    cs = _refs(n)[0]
    rw = _rotations(cs["points"]["xyz"].shape[0], 77)
    ref32, ref64, rv = _oracle_pair(cs, cs["pidx"], cs["campos"], cs["camrot"], cs["loc_p"], rw=rw)
    r = _run(cs, cuda, rw=rw)[0][0]
    assert np.array_equal(r["vmask"] != 0, rv) and not r["out"][~rv].any()
    _bound(r["out"][:, 0], ref32[:, 0], ref64[:, 0], f"alpha rw2c n={n}")
    _bound(r["out"], ref32, ref64, f"features rw2c n={n}")


def _two_cameras(cs):
    from pointnerf_amd import synthetic as S
    n = cs["pidx"].shape[0]
    cpb, crb = S.camera(75.0, -20.0, 4.0)
    cam = ((np.arange(n) // 3) % 2).astype(np.int32)
    loc_pb = O.w2pers(cs["loc_w"], cpb, crb).astype(np.float32)
    return cpb, crb, cam, loc_pb


@pytest.mark.parametrize("n", COUNTS)
def test_h2_producers_two_cameras_vs_oracle(cuda, n):
    """A ray_cam batch of two cameras (general kernel): each sample against the oracle under its own camera."""
    cs = _refs(n)[0]
    cpb, crb, cam, loc_pb = _two_cameras(cs)
    b32, b64, rv = _oracle_pair(cs, cs["pidx"], cpb, crb, loc_pb)
    sel = cam.astype(bool)[:, None]
    ref32, ref64 = np.where(sel, b32, cs["ref32"]), np.where(sel, b64, cs["ref64"])
    assert np.array_equal(rv, cs["rv"])
    cams = (np.stack([cs["campos"], cpb]), np.stack([cs["camrot"], crb]), cam, np.where(sel, loc_pb, cs["loc_p"]))
    r = _run(cs, cuda, cams=cams)[0][0]
    assert np.array_equal(r["vmask"] != 0, rv) and not r["out"][~rv].any()
    _bound(r["out"][:, 0], ref32[:, 0], ref64[:, 0], f"alpha two cameras n={n}")
    _bound(r["out"], ref32, ref64, f"features two cameras n={n}")


@pytest.mark.parametrize("n", COUNTS)
def test_h2_producers_camera_hoist(cuda, n):
    """One camera from the constants block == a ray_cam batch whose two cameras are that camera."""
    cs = _refs(n)[0]
    cam = ((np.arange(n) // 3) % 2).astype(np.int32)
    cams = (np.stack([cs["campos"]] * 2), np.stack([cs["camrot"]] * 2), cam, cs["loc_p"])
    _same(_run(cs, cuda, cams=cams)[0][0], _base(cuda, n, K), cs["rv"])


@pytest.mark.parametrize("k", [K, K5])
@pytest.mark.parametrize("n", COUNTS)
def test_h2_producers_tile_independence(cuda, n, k):
    """The sample list rotated by 24 samples (three 8-sample tiles; 5 samples: by
    24 mod 5), the result un-rotated: a sample's bits depend neither on its tile
    nor on the loop iteration that renders it."""
    cs = _refs(n)[0] if k == K else _refs_k5(n)[0]
    _same(_run(cs, cuda, k=k, roll=24)[0][0], _base(cuda, n, k), cs["rv"])


def test_h2_producers_deterministic(cuda):
    res, _ = _run(_refs(8323)[0], cuda, launches=3)
    for r in res:
        _same(r, _base(cuda, 8323, K), _refs(8323)[0]["rv"])
        assert np.array_equal(r["bits"], res[0]["bits"])


def test_h2_producers_range_flag(cuda):
    """block3.2 bias 1e6: the activations leave the f16 range and the specialised
    kernel's tail raises the flag; the clean run leaves it clear."""
    cs = _refs(2061)[0]
    _, agg = _run(cs, cuda)   # asserts the flag is clear
    assert agg.h2_range_ok()
    _, bad = _run(cs, cuda, mutate=lambda a: a.block3[2].bias.fill_(1e6), check_range=False)
    assert not bad.h2_range_ok()
