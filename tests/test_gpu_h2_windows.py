"""k_pairs_h2 with producer work moved into an activation-store window
(aggregate_x3.hip producer_loop, SW): the same instructions at another time, so
the moved LDS readers and writers are what can go wrong -- a PE plane written
late or read early, a tail reading a parked accumulator or a Wt / Sf slot of the
wrong tile.

Cases as tests/test_gpu_h2_acc2.py builds them (3001 points, samples with 1..8
neighbours and one with none), at sample counts
  5     one partial tile: the tail runs only in the epilogue
  2061  258 tiles on 256 workgroups: dynamic hand-out
  8323  1041 tiles: some workgroup runs at least 5 tiles, so the three Wt / Sf
        slots and both extras buffers are reused; not a multiple of 8

Checked: the K-summed features `hid` that k_pairs_h2 leaves in the scratch as
f16 (hi, lo) planes per 64-sample tile (put together again here: x = hi +
2^-11 lo), the [n, 129] output (alpha and the colour branch) and vmask.

Bound (the one test_gpu_x3.py and test_gpu_h2_acc2.py state), against the
oracle in float64 with the float32 oracle's own error as the yardstick, for
`hid` and for the output each:
  max |h2 - ref64| <= 2 max |ref32 - ref64| + 1e-7 max|ref64|
  rms              <= 1.5 rms(ref32 - ref64) + 1e-8 max|ref64|
The hid reference repeats oracle.aggregate's own steps up to the K sums with
the oracle's functions (oracle.aggregate returns only the final features); its
alpha must equal oracle.aggregate's bit for bit, which ties the two together."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_h2_acc2 import K, _case, _oracle_f64

pytestmark = pytest.mark.gpu
COUNTS = [5, 2061, 8323]


def _hid_oracle(cs, f64):
    """(hid [n_valid, 256], alpha [n_valid]) by oracle.aggregate's steps (lego
    configuration, no per-point rotation), in float32 or float64."""
    g = O.gather(cs["points"], cs["pidx"][:, None, :], cs["campos"], cs["camrot"])
    with _oracle_f64() if f64 else contextlib.nullcontext():
        F = O.F32
        prm = {k: v.astype(F) for k, v in cs["params"].items()}
        mask = np.asarray(g["sample_pnt_mask"], bool)
        n = mask.shape[0]
        rv = mask.any(-1).reshape(-1)
        sx, sxp = np.asarray(g["sampled_xyz"], F), np.asarray(g["sampled_xyz_pers"], F)
        sl, slw = np.asarray(cs["loc_p"][:, None, :], F), np.asarray(cs["loc_w"][:, None, :], F)
        xd = (sxp[..., 0] * sxp[..., 2]).astype(F) - (sl[:, :, None, 0] * sl[:, :, None, 2]).astype(F)
        yd = (sxp[..., 1] * sxp[..., 2]).astype(F) - (sl[:, :, None, 1] * sl[:, :, None, 2]).astype(F)
        zd = sxp[..., 2] - sl[:, :, None, 2]
        dists = np.concatenate([(sx - slw[..., None, :]).astype(F), np.stack([xd, yd, zd], -1).astype(F)], -1).astype(F)
        w = (1.0 / np.maximum(np.sqrt((dists[..., :3] ** 2).sum(-1)), F(1e-6))).astype(F)
        w = (mask * w).astype(F)
        w = (w / np.maximum(w.sum(-1, keepdims=True), F(1e-8))).astype(F)
        confc = np.clip(np.asarray(g["sampled_conf"], F)[..., 0], F(1e-4), F(1)).astype(F)
        wt = (w * confc).astype(F)
        Rw = np.eye(3, dtype=F)
        pm = mask.reshape(-1)
        vd = (np.asarray(cs["vd"], F).reshape(-1, 3) @ Rw.T).astype(F)
        ori_v = O.positional_encoding(vd, 4, ori=True)[:, :3]
        d = dists.reshape(-1, 6)[pm].copy()
        d[:, :3] = (d[:, :3] @ Rw.T).astype(F)
        d = O.positional_encoding(d, 5)
        e = np.asarray(g["sampled_embedding"], F).reshape(-1, 32)[pm]
        feat = np.concatenate([e, O.positional_encoding(e, 3), d], -1)
        feat = O._lrelu(O._lin(feat, prm, "block1.0"), 0.01)
        feat = O._lrelu(O._lin(feat, prm, "block1.2"), 0.01)
        col = np.asarray(g["sampled_color"], F).reshape(-1, 3)[pm]
        sdir = (np.asarray(g["sampled_dir"], F).reshape(-1, 3)[pm] @ Rw.T).astype(F)
        ov = np.repeat(ori_v[:, None, :], K, 1).reshape(-1, 3)[pm]
        feat = np.concatenate([feat, col, sdir - ov, (sdir * ov).sum(-1, keepdims=True)], -1).astype(F)
        feat = O._lrelu(O._lin(feat, prm, "block3.0"), 0.01)
        feat = O._lrelu(O._lin(feat, prm, "block3.2"), 0.01)
        a = O._softplus(O._lin(feat, prm, "alpha_branch.0") - 1)
        ah = np.zeros((n * K, 1), F)
        ah[pm] = a
        wv = wt.reshape(n, K, 1)
        alpha = (ah.reshape(n, K, 1) * wv).sum(-2)[rv]
        fh = np.zeros((n * K, feat.shape[-1]), F)
        fh[pm] = feat
        hid = (fh.reshape(n, K, -1) * wv).sum(-2)[rv].astype(F)
    return hid, alpha[:, 0]


@functools.lru_cache(maxsize=None)
def _refs(n):
    """The case, its hid references (float32, float64) and the check that they
    follow oracle.aggregate (computed once, read-only)."""
    cs = _case(n, "plain")
    h32, a32 = _hid_oracle(cs, False)
    h64, a64 = _hid_oracle(cs, True)
    assert h32.dtype == np.float32 and h64.dtype == np.float64
    assert np.array_equal(a32, cs["ref32"][cs["rv"], 0]) and np.array_equal(a64, cs["ref64"][cs["rv"], 0])
    h32.setflags(write=False)
    h64.setflags(write=False)
    return cs, h32, h64


def _run(cs, cuda, launches=1, mutate=None, check_range=True):
    """pnr_aggregate_fwd_h2 on zeroed scratch -> per launch (out [n, 129], the raw
    hid plane bytes, hid [n, 256] float64, vmask [n]); the aggregator."""
    from pointnerf_amd import _lib as L
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints
    pt = cs["points"]
    agg = PointAggregator(cs["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in cs["params"].items()})
    agg.eval()
    if mutate is not None:
        with torch.no_grad():
            mutate(agg)
    np_ = NeuralPoints(cs["opt"], cuda, *(torch.from_numpy(np.array(pt[k])) for k in ("xyz", "emb", "color", "dir", "conf")))
    dev = {k: torch.from_numpy(np.array(cs[k])).to(cuda).contiguous() for k in ("campos", "camrot", "pidx", "loc_w", "loc_p", "vd")}
    n = cs["pidx"].shape[0]
    s = L.Samples(None, None, n, dev["pidx"].data_ptr(), dev["loc_w"].data_ptr(), dev["loc_p"].data_ptr(),
                  dev["vd"].data_ptr(), None, 1, K)
    pts, _keep = np_.tables(dev["campos"], dev["camrot"])
    mlp, _k1 = agg.packed()
    mlph, _k2 = agg.packed_h2()
    # scratch = P1 [points, 256] | hid planes [tiles of 64 samples] | vmask (aggregate.hip carve)
    nm = -(-n // 64) * 64
    h0 = int(pts.n) * 256
    outs = []
    for _ in range(launches):
        f = torch.zeros((n, 129), device=cuda)
        scr = L.aggregate_scratch(n, pts.n, cuda).zero_()
        L.check(L.lib().pnr_aggregate_fwd_h2(L.ctypes.byref(pts), L.ctypes.byref(s), L.ctypes.byref(mlp),
                                             L.ctypes.byref(mlph), L.ptr(f), None, None, L.ptr(scr), scr.numel() * 4,
                                             L.stream_ptr(cuda)), "pnr_aggregate_fwd_h2")
        outs.append((f, scr))
    torch.cuda.synchronize()
    if check_range:
        assert agg.h2_range_ok()
    res = []
    for f, scr in outs:
        raw = scr[h0:h0 + nm * 256].cpu().numpy().view(np.float16).reshape(nm // 64, 2, 32, 64, 8)
        with np.errstate(invalid="ignore"):   # (the range-flag case holds inf halves)
            x = raw[:, 0].astype(np.float64) + raw[:, 1].astype(np.float64) / 2048.0   # [tile, row group, sample, 8]
        hid = x.transpose(0, 2, 1, 3).reshape(nm, 256)[:n]
        vmask = scr[h0 + nm * 256:h0 + nm * 256 + n].view(torch.int32).cpu().numpy()
        res.append((f.cpu().numpy(), raw, hid, vmask))
    return res, agg


def _bound(got, ref32, ref64, what):
    e32 = np.abs(ref32.astype(np.float64) - ref64)
    eh2 = np.abs(got.astype(np.float64) - ref64)
    scale = np.abs(ref64).max()
    r32, rh2 = np.sqrt((e32 ** 2).mean()), np.sqrt((eh2 ** 2).mean())
    print(f"\n{what}: max|ref| {scale:.3g}  err vs f64 (max, rms): fp32 oracle {e32.max():.3g} {r32:.3g}"
          f"  fp32h2 {eh2.max():.3g} {rh2:.3g}")
    assert eh2.max() <= 2.0 * e32.max() + 1e-7 * scale
    assert rh2 <= 1.5 * r32 + 1e-8 * scale


@pytest.mark.parametrize("n", COUNTS)
def test_h2_windows_oracle_bound(cuda, n):
    cs, h32, h64 = _refs(n)
    (out, _raw, hid, vmask), = _run(cs, cuda)[0]
    rv = cs["rv"]
    assert np.array_equal(vmask != 0, rv)
    assert not out[~rv].any() and not hid[~rv].any()   # samples without a neighbour stay unwritten
    _bound(hid[rv], h32, h64, f"hid n={n}")
    _bound(out[:, 0], cs["ref32"][:, 0], cs["ref64"][:, 0], f"alpha n={n}")
    _bound(out, cs["ref32"], cs["ref64"], f"features n={n}")


def test_h2_windows_deterministic(cuda):
    """Three launches on the same inputs: a race between the moved LDS writers /
    readers and the consumers would show as differing bits."""
    res, _ = _run(_refs(8323)[0], cuda, launches=3)
    out0, raw0, _, vm0 = res[0]
    for out, raw, _, vm in res[1:]:
        assert np.array_equal(raw.view(np.uint16), raw0.view(np.uint16))
        assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
        assert np.array_equal(vm, vm0)


@pytest.mark.parametrize("layer", ["block1", "block3"])
def test_h2_windows_range_flag(cuda, layer):
    """block3.2 (and block1.2) bias 1e6: activations leave the f16 range and the
    launch raises its range flag; the clean run of the same case leaves it 0."""
    cs = _refs(2061)[0]
    _, agg = _run(cs, cuda)   # asserts the flag is clear
    assert agg.h2_range_ok()
    _, bad = _run(cs, cuda, mutate=lambda a: getattr(a, layer)[2].bias.fill_(1e6), check_range=False)
    assert not bad.h2_range_ok()
