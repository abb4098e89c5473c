"""The aggregate forward kernels against the float64 restatement of
tests/aggregate_ref.py on hand-built sample lists: pnr_aggregate_fwd, _x3, _h2
(with the f16-split colour / P1 packs and without), _masked, _bf16 (pair buckets
off and on) and _bf16_hf, called through ctypes on synthetic buffers.

Every output is pre-filled with a finite canary and carries a canary tail: rows
that must stay untouched (v >= min(*n_dev, n_max), samples without a neighbour,
out_weight / out_conf rows outside the list) must be the canary bit for bit.

Bars.  Project bar, unchanged: |d| <= 1e-4 + 1e-4 |ref64| for fp32 / x3 / h2 /
masked; bf16: 2 % relative RMS and 5 % of the block's maximum.  Tight bar for
the fp32-accurate paths, per case and block (alpha, colour, weight, conf):
max |got - ref64| <= c * max(e_o32, 2^-22 max|ref64|), where e_o32 is the error
of the numpy fp32 oracle against the float64 one on the same case, measured on
the CPU (never a kernel's own error); c = 8, the margin a split-MFMA GEMM already
gets over an fp32 one (test_gemm_tn_h2_vs_torch): an MFMA-blocked sum and numpy's
pairwise sum are two orderings of the same 256- to 284-term dot products.

Measured on one MI355X over all 55 cases (60 runs per path with the out_weight =
NULL repeats, 46 pair-table twins for masked; every line of the run is in
profiles/aggregate_edges_ratios.txt).  Per path: the worst err / max(e_o32, 2^-22
max|ref64|) for alpha / colour / weight with its cases, then the worst err / project
bar for alpha / colour / weight with its cases -- two separate maxima, each over all
cases (conf is exact on every path):
  fp32            2.10 / 1.51 / 0.57  (slots_xavier, count_64, count_1)
                  0.0005 / 0.0166 / 0.0006  (slots_xavier, geom_xavier, sched_4217)
  x3              1.26 / 1.81 / 0.42  (geom_xavier, rw2c_uniform, count_63)
                  0.0004 / 0.0184 / 0.0006  (ndev_2050, slots_xavier, sched_4217)
  h2              2.01 / 2.54 / 0.42  (act_lego, K_3, count_63)
                  0.0005 / 0.0152 / 0.0006  (act_lego, act_lego, sched_4217)
  h2, fp32 colour 1.72 / 1.51 / 0.42  (act_lego, count_64, count_63)
                  0.0004 / 0.0159 / 0.0006  (sched_4249, act_lego, sched_4217)
  masked          3.00 / 1.62 / 0.57  (slots_xavier, count_64, count_1)
                  0.0009 / 0.0182 / 0.0006  (slots_xavier, geom_xavier, list_dirmap)
The colour block's 1.5 to 1.8 % of the project bar comes from the xavier cases (max|ref|
2.4 to 4), where the numpy fp32 oracle's own noise is 1.2 to 2.0 % of the bar.
No path needs more than c = 8 (the worst is 3.0), so c stays 8 for all of them: h2's
dropped 2^-22 Wl.Xl term and the 1e-6 clamp of the coincident-point cases do not show
at this margin.  bf16 (b0 / b1 / hf): worst 1.1 % relative RMS (count_15) and 2.7 % of
the maximum (ntail_63); buckets on against off: 0 of 255 291 pooled entries differ.

Found by the h2 run with wc1a / w1ah NULL, on every case: the inference k_pairs_h2
leaves hid as f16-split planes and the fp32 k_color read them as fp32 rows (colour up
to 1.9e5 times the project bar); fixed by k_hid_rows_h2.
"""
import numpy as np
import pytest
import torch

import aggregate_ref as AR

pytestmark = pytest.mark.gpu

# c of the tight bar per path (see the module docstring)
C_PATH = {"fp32": AR.C_TIGHT, "x3": AR.C_TIGHT, "h2": AR.C_TIGHT, "h2_f32colour": AR.C_TIGHT, "masked": AR.C_TIGHT}
SPLIT_PATHS = ("fp32", "x3", "h2", "h2_f32colour")
BF16_PATHS = ("bf16_b0", "bf16_b1", "bf16_hf")
HF_FILL = 0x4442          # int16 canary of the bf16 feature rows (a finite bf16, a finite fp32 pair)
SCRATCH_JUNK = 7.0        # stale scratch is finite junk, never zeros
WORST = {}                # (path, block) -> [worst err / noise, its case, worst err / project bar, its case]
_AGGS = {}


def _agg(c, cuda):
    """The aggregator of a case's weight set (cached: the packs are built once)."""
    from pointnerf_amd.aggregator import PointAggregator
    key = (c.weights, c.neg_slope, c.act_super, None if c.Rw2c is None else c.Rw2c.tobytes())
    if key not in _AGGS:
        agg = PointAggregator(AR.opt_of(c)).to(cuda)
        agg.load_state_dict({k: torch.from_numpy(v) for k, v in AR.params_of(c).items()})
        if c.Rw2c is not None:
            with torch.no_grad():
                agg.rw2c.copy_(torch.from_numpy(np.array(c.Rw2c)))
        _AGGS[key] = agg.eval()
    return _AGGS[key]


class Dev:
    """A case on the device: its tensors (kept alive here), pnr_points and pnr_samples.
    use_used False drops the used subset; samp_list / n_max / n_dev override the list."""

    def __init__(self, c, cuda, use_used=True, samp_list="case", n_max=None, n_dev="case"):
        from pointnerf_amd import _lib as L
        self.c, self.cuda = c, cuda
        up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(cuda)   # noqa: E731
        t = self.t = {k: up(getattr(c, k)) for k in ("xyz", "pers", "emb", "color", "dir", "conf", "campos", "camrot",
                                                      "rw2c", "ray_cam", "pidx", "pair_mask", "sample_w", "sample_p",
                                                      "dirs", "dir_map")}
        used = use_used and c.used is not None
        t["used"] = up(c.used) if used else None
        t["used_map"] = up(c.used_map) if used else None
        t["n_used_dev"] = (torch.tensor([c.n_used_dev], dtype=torch.int32, device=cuda)
                           if used and c.n_used_dev is not None else None)
        sl = c.samp_list if isinstance(samp_list, str) else samp_list
        t["samp_list"] = up(None if sl is None else np.asarray(sl, np.int32))
        self.n_max = int(c.n_max if n_max is None else n_max)
        nd = c.n_dev if isinstance(n_dev, str) else n_dev
        # a NULL n_dev (every entry valid) where the case says so anyway, on the odd-sized lists
        t["n_dev"] = (None if nd is None or (nd == self.n_max and sl is None and c.rows % 2 == 1)
                      else torch.tensor([nd], dtype=torch.int32, device=cuda))
        self.n_p1 = int(c.used.shape[0]) if used else int(c.N)
        p = L.Points(c.N, L.ptr(t["xyz"]), L.ptr(t["pers"]), L.ptr(t["emb"]), L.ptr(t["color"]), L.ptr(t["dir"]),
                     L.ptr(t["conf"]), L.ptr(t["campos"]), L.ptr(t["camrot"]), L.ptr(t["used"]),
                     self.n_p1 if used else 0, L.ptr(t["used_map"]), 0, None, L.ptr(t["rw2c"]), L.ptr(t["n_used_dev"]))
        s = L.Samples(L.ptr(t["samp_list"]), L.ptr(t["n_dev"]), self.n_max, L.ptr(t["pidx"]), L.ptr(t["sample_w"]),
                      L.ptr(t["sample_p"]), L.ptr(t["dirs"]), L.ptr(t["dir_map"]), int(c.dir_div), int(c.K),
                      L.ptr(t["ray_cam"]))
        self.pts, self.s = p, s

    def outputs(self, hf=False):
        c, dev = self.c, self.cuda
        if hf:
            f = torch.full((self.n_max + AR.TAIL, 136), HF_FILL, dtype=torch.int16, device=dev)
        else:
            f = torch.full((self.n_max + AR.TAIL, 129), AR.CANARY_FEAT, device=dev)
        return (f, torch.full((c.rows + AR.TAIL, c.K), AR.CANARY_W, device=dev),
                torch.full((c.rows + AR.TAIL, c.K), AR.CANARY_C, device=dev))

    def scratch(self, bf16=False, n_max=None):
        from pointnerf_amd import _lib as L
        fn = L.aggregate_scratch_bf16 if bf16 else L.aggregate_scratch
        scr = fn(self.n_max if n_max is None else n_max, self.n_p1, self.cuda)
        scr.fill_(SCRATCH_JUNK)
        return scr


def _h2_pack(agg, path):
    from pointnerf_amd import _lib as L
    mh, keep = agg.packed_h2()
    if path == "h2_f32colour":   # wc1a and w1ah NULL: the fp32 colour branch and the fp32 k_point_pre
        mh = L.MlpH2.from_buffer_copy(mh)
        mh.wc1a = mh.wc1b = mh.wc2h = mh.wc3h = None
        mh.w1ah = None
    return mh, keep


def _decode_hf(fh):
    """bf16 feature rows -> [n, 129] float32 with whole untouched rows as the fp32
    canary; the unused slots 2..7 must keep their fill."""
    fh = fh.cpu()
    assert bool((fh[:, 2:8] == HF_FILL).all()), "bf16 rows: unused slots written"
    out = torch.empty((fh.shape[0], 129), dtype=torch.float32)
    out[:, 0] = fh[:, :2].contiguous().view(torch.float32)[:, 0]
    out[:, 1:] = fh[:, 8:136].contiguous().view(torch.bfloat16).float()
    alpha_u = (fh[:, :2] == HF_FILL).all(1)
    feat_u = (fh[:, 8:] == HF_FILL).all(1)
    assert torch.equal(alpha_u, feat_u), "bf16 rows: alpha written without features or the reverse"
    out[alpha_u] = AR.CANARY_FEAT
    return out.numpy()


def run(path, d, agg, with_wc=True, scr=None, p1_ready=0):
    """One call of ``path`` on canary-prefilled outputs -> (feat, weight | None, conf | None) numpy."""
    from pointnerf_amd import _lib as L
    lib, by = L.lib(), L.ctypes.byref
    hf = path == "bf16_hf"
    f, w, c = d.outputs(hf)
    wp, cp = (L.ptr(w), L.ptr(c)) if with_wc else (None, None)
    d.pts.p1_ready = int(p1_ready)
    st = L.stream_ptr(d.cuda)
    if path.startswith("bf16"):
        m16, _k16 = agg.packed_bf16()
        m16 = L.MlpBf16.from_buffer_copy(m16)
        m16.pair_buckets = int(path == "bf16_b1" or hf)
        scr = d.scratch(bf16=True) if scr is None else scr
        fn = lib.pnr_aggregate_fwd_bf16_hf if hf else lib.pnr_aggregate_fwd_bf16
        L.check(fn(by(d.pts), by(d.s), by(m16), L.ptr(f), wp, cp, L.ptr(scr), scr.numel() * 4, st), path)
    else:
        mlp, _k = agg.packed()
        scr = d.scratch() if scr is None else scr
        tail = (L.ptr(f), wp, cp, L.ptr(scr), scr.numel() * 4, st)
        if path == "fp32":
            L.check(lib.pnr_aggregate_fwd(by(d.pts), by(d.s), by(mlp), *tail), path)
        elif path == "masked":
            L.check(lib.pnr_aggregate_fwd_masked(by(d.pts), by(d.s), by(mlp), L.ptr(d.t["pair_mask"]), *tail), path)
        elif path == "x3":
            mx, _kx = agg.packed_x3()
            L.check(lib.pnr_aggregate_fwd_x3(by(d.pts), by(d.s), by(mlp), by(mx), *tail), path)
        else:
            mh, _kh = _h2_pack(agg, path)
            L.check(lib.pnr_aggregate_fwd_h2(by(d.pts), by(d.s), by(mlp), by(mh), *tail), path)
    torch.cuda.synchronize()
    d.pts.p1_ready = 0
    if path.startswith("h2"):
        assert agg.h2_range_ok(), f"{d.c.name}: h2 range flag raised"
    feat = _decode_hf(f) if hf else f.cpu().numpy()
    return feat, (w.cpu().numpy() if with_wc else None), (c.cpu().numpy() if with_wc else None)


def _note(path, name, res, e, sc):
    """Print err, e_o32, err / noise and err / project bar per block; keep the worst."""
    out = {}
    for k, err in res["err"].items():
        noise = max(e[k], AR.ULP_FLOOR * sc[k])
        r = err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))
        out[k] = r
        print(f"RATIO {path:13s} {name:18s} {k:7s} err {err:.3e}  e_o32 {e[k]:.3e}  err/noise {r:8.3f}  "
              f"err/bar {res['bar_ratio'][k]:.5f}")
        b = res["bar_ratio"][k]
        w = WORST.setdefault((path, k), [-1.0, name, -1.0, name])   # the two maxima, each with its own case
        if r > w[0]:
            w[0], w[1] = r, name
        if b > w[2]:
            w[2], w[3] = b, name
    return out


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nWORST err / max(e_o32, 2^-22 max|ref64|) and err / project bar per path and block")
    for (path, k), (r, rname, b, bname) in sorted(WORST.items()):
        print(f"WORST {path:13s} {k:7s} err/noise {r:8.3f} ({rname})  err/bar {b:.5f} ({bname})")


def _check_fp32_accurate(path, name, d, agg, masked=False, with_wc=True):
    c = d.c
    ref, e, sc, _ = AR.ref64_and_noise(name, masked)
    got = run(path, d, agg, with_wc)
    again = run(path, d, agg, with_wc)
    for a, b in zip(got, again):
        assert a is None or np.array_equal(a, b), f"{path} {name}: two runs differ"
    res = AR.compare(c, ref, *got)
    assert not res["canary"], (path, name, res["canary"])
    ratios = _note(path, name, res, e, sc)
    fails = [(k, res["bar_ratio"][k]) for k in ratios if res["bar_ratio"][k] > 1.0]
    assert not fails, f"{path} {name}: over the project bar {fails}"
    tight = [(k, r) for k, r in ratios.items() if r > C_PATH[path]]
    assert not tight, f"{path} {name}: err / max(e_o32, 2^-22 max|ref|) over c = {C_PATH[path]}: {tight}"


# with_wc False: out_weight / out_conf NULL (the render path) on the tile-edge counts
@pytest.mark.parametrize("name, with_wc", [(n, True) for n in AR.CASES] +
                         [(n, False) for n in ("count_9", "count_65", "count_129", "slots", "sched_4217")])
def test_fp32_accurate_paths_vs_fp64(cuda, name, with_wc):
    """pnr_aggregate_fwd, _x3, _h2 (f16-split colour and P1 packs) and _h2 with wc1a / w1ah
    NULL: canaries, the project bar, the tight bar, two runs bitwise equal, h2 range flag."""
    c = AR.case(name)
    d, agg = Dev(c, cuda), _agg(c, cuda)
    for path in SPLIT_PATHS:
        _check_fp32_accurate(path, name, d, agg, with_wc=with_wc)


@pytest.mark.parametrize("name", AR.MASKED)
def test_masked_vs_fp64(cuda, name):
    """pnr_aggregate_fwd_masked on the same cases pre-gathered to [rows * K, C] tables
    with pair_mask (one camera, pers given)."""
    c = AR.to_masked(AR.case(name))
    _check_fp32_accurate("masked", name, Dev(c, cuda), _agg(c, cuda), masked=True)


def _bf16_bar(name, path, c, ref, got):
    res = AR.compare(c, ref, *got)
    assert not res["canary"], (path, name, res["canary"])
    wr = ~ref["untouched"]
    for blk, sl in (("alpha", slice(0, 1)), ("colour", slice(1, 129))):
        w = ref["feat"][wr][:, sl]
        if not w.size or np.abs(w).max() == 0.0:
            continue
        dlt = got[0][:c.n_max][wr][:, sl].astype(np.float64) - w
        rms = float(np.sqrt((dlt ** 2).mean() / (w ** 2).mean()))
        mx = float(np.abs(dlt).max() / np.abs(w).max())
        print(f"BF16  {path:13s} {name:18s} {blk:7s} rel rms {rms:.4f}  max / max|ref| {mx:.4f}")
        assert rms < 0.02 and mx <= 0.05, (path, name, blk, rms, mx)
    for blk in ("weight", "conf"):   # fp32 arithmetic on every path
        assert res["bar_ratio"][blk] <= 1.0, (path, name, blk, res["bar_ratio"][blk])


@pytest.mark.parametrize("name", AR.CASES)
def test_bf16_paths_vs_fp64(cuda, name):
    """pnr_aggregate_fwd_bf16 with pair_buckets 0 and 1 and pnr_aggregate_fwd_bf16_hf:
    canaries, the bf16 bar against float64 (hole patterns included, both bucket
    settings), two runs bitwise equal."""
    c = AR.case(name)
    d, agg = Dev(c, cuda), _agg(c, cuda)
    ref = AR.ref64_and_noise(name)[0]
    for path in BF16_PATHS:
        got = run(path, d, agg)
        again = run(path, d, agg)
        for a, b in zip(got, again):
            assert np.array_equal(a, b), f"{path} {name}: two runs differ"
        _bf16_bar(name, path, c, ref, got)


def test_bf16_buckets_on_against_off(cuda):
    """Pair buckets on against off over every small case (pooled entries): the same
    rows written, alpha within 2^-20 of its maximum, at most 0.1 % of the entries apart
    and those by at most 2^-7 of the maximum -- the contract of test_gpu_bf16.py, not
    bitwise (two instantiations of k_pairs_b)."""
    n_diff = n_all = 0
    for name in AR.SMALL:
        c = AR.case(name)
        d, agg = Dev(c, cuda), _agg(c, cuda)
        a, wa, ca = run("bf16_b0", d, agg)
        b, wb, cb = run("bf16_b1", d, agg)
        assert np.array_equal(a == AR.CANARY_FEAT, b == AR.CANARY_FEAT), name
        assert np.array_equal(wa, wb) and np.array_equal(ca, cb), name
        wr = a[:, 0] != AR.CANARY_FEAT
        if not wr.any():
            continue
        dl = np.abs(a[wr].astype(np.float64) - b[wr])
        assert dl[:, 0].max() <= 2.0 ** -20 * np.abs(a[wr, 0]).max(), (name, dl[:, 0].max())
        assert dl.max() <= 2.0 ** -7 * np.abs(a[wr]).max(), (name, dl.max())
        n_diff += int((dl > 0).sum())
        n_all += dl.size
    print(f"buckets on against off: {n_diff} of {n_all} entries differ ({n_diff / n_all:.2e})")
    assert n_diff <= 1e-3 * n_all


@pytest.mark.parametrize("path", ["fp32", "x3", "h2"])
@pytest.mark.parametrize("name", ["list_perm", "sched_4217"])
def test_permuting_the_list_permutes_the_rows(cuda, path, name):
    """A sample's bits depend on neither its tile nor its place in the tile."""
    c = AR.case(name)
    agg = _agg(c, cuda)
    base = np.arange(c.n_max, dtype=np.int32) if c.samp_list is None else c.samp_list
    perm = np.random.default_rng(7).permutation(c.n_max)
    fa, wa, ca = run(path, Dev(c, cuda, samp_list=base), agg)
    fb, wb, cb = run(path, Dev(c, cuda, samp_list=base[perm]), agg)
    assert np.array_equal(fb[:c.n_max], fa[:c.n_max][perm])
    assert np.array_equal(wa, wb) and np.array_equal(ca, cb)   # indexed by sample row


@pytest.mark.parametrize("path", ["fp32", "x3", "h2"])
@pytest.mark.parametrize("name", ["used_subset", "used_dev"])
def test_used_subset_equals_full_table(cuda, path, name):
    c = AR.case(name)
    agg = _agg(c, cuda)
    a = run(path, Dev(c, cuda, use_used=True), agg)
    b = run(path, Dev(c, cuda, use_used=False), agg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["count_129", "used_subset", "ntail_65"])
def test_h2_point_pre_then_p1_ready(cuda, name):
    """pnr_point_pre_h2 into the scratch, then pnr_aggregate_fwd_h2 with p1_ready = 1,
    equals the one call."""
    from pointnerf_amd import _lib as L
    c = AR.case(name)
    d, agg = Dev(c, cuda), _agg(c, cuda)
    one = run("h2", d, agg)
    scr = d.scratch()
    mh, _keep = agg.packed_h2()
    L.check(L.lib().pnr_point_pre_h2(L.ctypes.byref(d.pts), L.ctypes.byref(mh), L.ptr(scr), scr.numel() * 4,
                                     L.stream_ptr(cuda)), "pnr_point_pre_h2")
    two = run("h2", d, agg, scr=scr, p1_ready=1)
    for x, y in zip(one, two):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n_first, n_second", [(129, 65), (65, 129), (129, 8)])
def test_h2_second_call_other_n_max_same_scratch(cuda, n_first, n_second):
    """P1 sits at the head of the scratch, so a second call with another n_max and
    p1_ready = 1 on the same scratch equals a fresh call."""
    c = AR.case("count_129")
    agg = _agg(c, cuda)
    first, second = Dev(c, cuda, n_max=n_first, n_dev=None), Dev(c, cuda, n_max=n_second, n_dev=None)
    scr = first.scratch(n_max=129)
    run("h2", first, agg, scr=scr)
    again = run("h2", second, agg, scr=scr, p1_ready=1)
    fresh = run("h2", second, agg)
    for x, y in zip(again, fresh):
        assert np.array_equal(x, y)
    ref = AR.ref64_and_noise("count_129")[0]
    wr = ~ref["untouched"][:n_second]
    assert np.allclose(again[0][:n_second][wr], ref["feat"][:n_second][wr], atol=AR.ATOL, rtol=AR.RTOL)
    assert np.all(again[0][n_second:] == AR.CANARY_FEAT)
