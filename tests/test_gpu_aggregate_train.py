"""The training aggregate (pnr_aggregate_fwd_train, _x3, _h2_guarded, _masked) and the
whole backward behind train.AggregateFn against the pinned-sign float64 restatement
of tests/aggregate_train_ref.py, on the hand-built sample lists of
tests/aggregate_ref.py (every small case and sched_4217 / ndev_2050), through
``AggSpec(keep_saved=True)`` and the ``Dev`` class of the forward suite.

Kinks are pinned: the backward never recomputes a LeakyReLU sign, it reads the
forward's saves, so the reference takes every branch from the kernel's own saved
post-activations and the comparison is arithmetic alone.  That the saved signs are
right is part (a): a saved sign may differ from ``z64 > 0`` only where |z64| <=
8 max(e_o32(layer), 2^-22 max|z64(layer)|).

Parts (each a test function over the same runs):
  (a) the training forward: feat against aggregate_ref.reference (float64) under the
      forward suite's two bars; the saves prow / vmask / wt / wn / pe5 / x3e / hid;
      the pinning condition; the mask words against ``saved h > 0``;
  (b) the pairs chain, where the Python sequence ran: dz1..dz4, dpa and the per-pair
      d conf; rows of empty pairs and of the slots K..7 exactly 0;
  (c) d emb / d colour / d dir / d conf; rows of unreferenced points exactly 0; two
      backward runs bitwise equal; the native step bitwise the Python sequence;
  (d) the 16 parameter gradients;
  (e) d xyz (every case but pers_given and the pair-table twins).

Bars for (b)-(e), per tensor and case: max |got - g64| <= c max(e_o32, 2^-22 max|g64|),
e_o32 = the restatement's float32 run against its float64 run under the kernel's
signs, measured on the CPU.  c = 8 on every path (``C_PATH``), fp32h2 included, for
every tensor but two bias column sums, each on the paths that measured over 8 only
(``C_TENSOR``, keyed by path and tensor, c = 32, below).

Measured on one MI355X over the 208 runs (profiles/aggregate_train_ratios.txt: every ratio,
the RATIO lines of a ``pytest -s`` run condensed by tools/ratio_table.py to one row per path
and case, and the WORST table).  Worst err / max(e_o32, 2^-22 max|g64|) per
path, with its case -- fp32 / fp32x3 / fp32h2 / masked:
  feat alpha, colour        2.10, 1.51 / 1.26, 1.81 / 2.03, 2.25 / 3.00, 1.62
  dz1 dz2 dz3 dz4           2.35 1.78 1.32 1.36 / 2.58 1.80 1.42 1.36 / 2.37 2.17 1.84 1.64 / 2.35 1.78 1.30 1.36
  dpa, per-pair d conf      2.17, 1.62 / 2.16, 2.16 / 3.10, 1.56 / 2.62, 1.80
  d emb                     3.74 (count_17) / 2.86 (K_1) / 2.56 (count_17) / 4.06 (count_17)
  d colour, d dir           2.75, 1.84 / 5.14, 6.64 (ntail_1) / 3.53, 4.25 (ntail_1) / 2.76, 1.70
  d conf                    1.82 / 2.10 / 1.56 / 1.80
  d xyz                     7.70 (ndev_250) / 4.87 (ndev_250) / 2.03 (count_1) / -
  weights, worst            2.85 alpha_branch.0 (ndev_2050) / 6.96 block1.2 (sched_4217) /
                            5.71 block1.2 (sched_4217) / 2.85 alpha_branch.0 (count_63)
  biases but the two below  2.27 block1.0 / 6.71 block1.0 (sched_4217) / 3.98 block1.0 (sched_4217) / 2.12 block1.0
  d block1.2.bias           2.07 (count_1) / 13.89 (ndev_2050) / 11.25 (ndev_2050) / 2.07
  d alpha_branch.0.bias     8.31 (color_null) / 8.31 (color_null) / 9.08 (dir_null) / 8.16 (color_null)
So with the kinks pinned fp32h2's gradients sit at 1 to 6 times the noise of fp32 arithmetic,
like fp32's and fp32x3's own: the per-cent differences of
test_train_h2_grads_vs_x3 are LeakyReLU branch flips, not arithmetic.  Saved signs that differ
from z64 > 0: at most 4 of 4.7 M entries per layer (sched_4217), every one within the bar.
d xyz on ndev_250 (fp32 7.70, fp32x3 4.65 to 4.87 from run to run: float atomics) is one entry,
point 237's z, at 3e-6 of its value; the next largest row error is a tenth of it.

The two tensors over c = 8, which get c = 32 (the worst measured ratio doubled, rounded up to
a power of two) on the paths where they are over it -- the first on all four, the second on
fp32x3 and fp32h2 only (fp32 and masked keep c = 8 for it) -- are sums over every pair of the
list with cancellation:
  * d alpha_branch.0.bias is ONE number, sum(dpa) -- 264 terms of up to 0.5 that cancel to
    7e-3 on color_null -- so its e_o32 is a single draw of the CPU's own rounding (1.6e-8, half
    an ulp of a term) and the kernel's 1.4e-7 (four ulps of a term, torch's device sum) is
    8.3 times it, the same on all three paths;
  * d block1.2.bias on the two big lists (34 k pairs) on fp32x3 and fp32h2 only (fp32: 0.7 and
    2.0 through the same pnr_gemm_tn_x3 column sum, so the sum is not the cause): dz2 is the
    output of the block3.0^T GEMM of k_pairs_bwd<1|2> on split operands; per entry it is within
    1.8 to 2.2 times noise, but over 34 k pairs its error does not average out the way the fp32
    chain's does (supposed: the dropped low products of the splits are correlated with the
    weights, not independent per pair); block1.2.weight (7.0 / 5.7) and block1.0.bias (6.7 / 4.0)
    show the same on those two lists.  It is 1.7e-5 of the tensor's largest entry.

Found by this suite: two backward runs of train_precision fp32 differed in d colour / d dir
(count_63: the fp32 pairs kernel added them with float atomics); every chain now sums them per
point in pair order.  ndev_0 with an xyz gradient failed with "aggregate_bwd_xyz: null
argument" (an empty list has no d PE_5 rows); d xyz is now 0 there without a launch.

Also here: pnr_group_pairs at the group-size edges (1 .. 5000 pairs per key; the call with the
5000-pair group takes 3.8 ms for 7154 pairs, the quadratic rank of k_grp_sort_big) and the
atomic form of pnr_aggregate_bwd_pairs (d_p1 given), which no other test calls.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aggregate_ref as AR
import aggregate_train_ref as TR
from test_gpu_aggregate_edges import Dev, _agg

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp32x3", "fp32h2")
BIG = ("sched_4217", "ndev_2050")
C_PATH = {"fp32": 8.0, "fp32x3": 8.0, "fp32h2": 8.0, "masked": 8.0}
# the two column sums over every pair that need more than c = 8, on the paths where they measured over
# it (module docstring): the alpha bias on all four, block1.2's bias on the split chains only
C_TENSOR = {(p, "d alpha_branch.0.bias"): 32.0 for p in C_PATH}
C_TENSOR.update({(p, "d block1.2.bias"): 32.0 for p in ("fp32x3", "fp32h2")})
RUNS = ([(n, p, False) for n in AR.SMALL + BIG for p in PRECISIONS] + [(n, "fp32", True) for n in AR.MASKED])
WORST = {}    # (path, tensor) -> [worst err / noise, its case]


def _np(t):
    return t.detach().cpu().numpy()


class Run:
    """One case on one path: the forward with its saves, the backward (the stages spied
    on), and the pinned reference with its noise.  Everything is made once, on demand."""

    def __init__(self, name, prec, masked, cuda):
        self.name, self.prec, self.masked, self.cuda = name, prec, masked, cuda
        self.path = "masked" if masked else prec
        self.case = AR.case(name)
        self.c = AR.to_masked(self.case) if masked else self.case
        self.n = max(0, min(int(self.c.n_dev), int(self.c.n_max)))
        self.xyz_ok = self.c.pers is None
        self._memo = {}

    # ------------------------------------------------------------------ the kernels
    def execute(self, xyz_grad=False, native=True):
        """feat = AggregateFn.apply(...); feat.backward(G) -> dict of numpy results."""
        import pointnerf_amd.train as T
        key = (xyz_grad, native)
        if key in self._memo:
            return self._memo[key]
        c, cuda = self.c, self.cuda
        d, agg = Dev(c, cuda), _agg(c, cuda)
        t = d.t
        used = counts = None
        if t["used"] is not None:
            cnt = t["n_used_dev"]
            if cnt is None:
                cnt = torch.tensor([c.used.shape[0]], dtype=torch.int32, device=cuda)
            used = T.UsedPoints(t["used"], t["used_map"], cnt)
            if c.n_used_dev is not None:   # capacities with the counts on the device: the backward reads them
                got = {"S_valid": self.n, "n_used": int(c.n_used_dev)}
                counts = SimpleNamespace(get=lambda: got)
        leaf = {"emb": t["emb"].clone().requires_grad_(True)}
        for k in ("color", "dir"):
            leaf[k] = None if t[k] is None else t[k].clone().requires_grad_(True)
        leaf["conf"] = None if t["conf"] is None else t["conf"].reshape(-1, 1).clone().requires_grad_(True)
        xyz = t["xyz"].clone().requires_grad_(True) if xyz_grad else None
        tabs = T.PointTables(t["xyz"] if xyz is None else xyz.detach(), pers=t["pers"], campos=t["campos"],
                             camrot=t["camrot"], rw2c=None if t["rw2c"] is None else t["rw2c"].reshape(-1, 9))
        spec = T.AggSpec(agg, d.s, self.n, tabs, pair_mask=t["pair_mask"] if self.masked else None, used=used,
                         precision=self.prec, counts=counts, keep=(d,), keep_saved=True)
        params = T.agg_params(agg)
        for p in params:
            p.grad = None
        ran = dict(python=0, native=0, stages=None)

        class Spy(T._Backward):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                ran["python"] += 1
                ran["stages"] = self

        real_native = T._native_bwd_h2

        def spy_native(*a, **kw):
            ran["native"] += 1
            return real_native(*a, **kw)

        old = T._Backward, T._native_bwd_h2, T.NATIVE_BWD
        T._Backward, T._native_bwd_h2, T.NATIVE_BWD = Spy, spy_native, native
        try:
            feat = T.AggregateFn.apply(spec, leaf["emb"], leaf["color"], leaf["dir"], leaf["conf"], xyz, *params)
            G = torch.from_numpy(TR.upstream(c)).float().to(cuda)
            assert feat.shape == G.shape, (feat.shape, G.shape)
            feat.backward(G)
            torch.cuda.synchronize()
        finally:
            T._Backward, T._native_bwd_h2, T.NATIVE_BWD = old
        if self.prec == "fp32h2":
            assert not agg.h2_train_poll(wait=True), f"{self.name}: the h2 range flag was raised (fp32 fallback ran)"
        out = dict(feat=_np(feat), ran=ran, spec=spec, n_used=None if used is None else int(cnt.item()))
        out["grads"] = {k: (None if v is None else _np(v.grad).reshape(v.shape[0], -1)) for k, v in leaf.items()}
        out["grads"]["xyz"] = None if xyz is None else _np(xyz.grad)
        for k, p in zip(TR.PARAM_NAMES, params):
            out["grads"][k] = _np(p.grad)
            p.grad = None
        self._memo[key] = out
        return out

    @property
    def main(self):
        return self.execute()

    def saves(self):
        """The forward's kept activations of the rows [0, n): numpy, pairs as [n, 8, ...]."""
        if "saves" not in self._memo:
            sv, n = self.main["spec"].saved, self.n
            o = {}
            for k in ("h1", "h2", "h3", "h4", "pe5", "x3e", "mask"):
                o[k] = _np(sv[k][:n * 8]).reshape(n, 8, -1)
            for k in ("pa", "wt", "wn", "prow"):
                o[k] = _np(sv[k][:n * 8]).reshape(n, 8)
            for k in ("hid", "hc1", "hc2", "hc3", "vmask"):
                o[k] = _np(sv[k][:n])
            self._memo["saves"] = o
        return self._memo["saves"]

    def signs(self):
        s, K = self.saves(), self.c.K
        sg = {k: s[k][:, :K] > 0 for k in ("h1", "h2", "h3", "h4")}
        sg.update({k: s[k] > 0 for k in ("hc1", "hc2", "hc3")})
        sg["pa"] = s["pa"][:, :K] > 0
        return sg

    def ref(self):
        """(r64, e_o32, scale) of the restatement under the kernel's saved signs."""
        if "ref" not in self._memo:
            self._memo["ref"] = TR.noise(self.case, self.signs() if self.n else None, xyz_grad=self.xyz_ok,
                                         masked=self.masked)
        return self._memo["ref"]

    # ------------------------------------------------------------------ the bar
    def check(self, tensors):
        """tensors: name -> (got, key in the reference's grads).  Prints one RATIO line per
        tensor and asserts err <= c max(e_o32, 2^-22 max|g64|) on each (c: C_TENSOR, else C_PATH)."""
        r64, e, sc = self.ref()
        over = []
        for tname, (got, key) in tensors.items():
            g64 = r64["grads"][key].reshape(got.shape)
            assert np.isfinite(got).all(), (self.path, self.name, tname, "not finite")
            err = float(np.abs(got.astype(np.float64) - g64).max()) if g64.size else 0.0
            noise = max(e[key], AR.ULP_FLOOR * sc[key])
            r = err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))
            print(f"RATIO {self.path:7s} {self.name:18s} {tname:22s} err {err:.3e}  e_o32 {e[key]:.3e}  "
                  f"max|g64| {sc[key]:.3e}  err/noise {r:8.3f}")
            w = WORST.setdefault((self.path, tname), [-1.0, self.name])
            if r > w[0]:
                w[0], w[1] = r, self.name
            c = C_TENSOR.get((self.path, tname), C_PATH[self.path])
            if r > c:
                over.append((tname, r, c))
        assert not over, f"{self.path} {self.name}: err / max(e_o32, 2^-22 max|g64|) over c (tensor, ratio, c): {over}"


@pytest.fixture(scope="module", params=RUNS, ids=lambda p: f"{p[0]}-{'masked' if p[2] else p[1]}")
def R(request, cuda):
    return Run(*request.param, cuda)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nWORST err / max(e_o32, 2^-22 max|g64|) per path and tensor")
    for (path, k), (r, name) in sorted(WORST.items()):
        print(f"WORST {path:7s} {k:22s} err/noise {r:8.3f} ({name})")


def _close(a, ref, name, rel, scale):
    """test_gpu_backward.close: |d| <= scale max|ref| + rel |ref|."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if not ref.size:
        return
    tol = scale * max(float(np.abs(ref).max()), 1e-30) + rel * np.abs(ref)
    bad = np.abs(a - ref) > tol
    assert not bad.any(), f"{name}: {bad.sum()} / {bad.size} outside tol, max |d| {np.abs(a - ref).max():.3e}"


def _mask_bits(words):
    """pnr_agg_saved.mask [n, 8, 64] int16 -> [n, 8, 4, 256] bool (layer, neuron), by the
    layout of pnr.h: word 16 l + 2T + h, bit r = register r of neuron tile T, lane half h."""
    w = (words.astype(np.int64) & 0xFFFF).reshape(words.shape[:2] + (4, 16))
    out = np.zeros(w.shape[:2] + (4, 256), bool)
    for word in range(16):
        for bit in range(16):
            out[:, :, :, TR.mask_neuron(word, bit)] = ((w[:, :, :, word] >> bit) & 1) != 0
    return out


# ------------------------------------------------------------------ (a) forward and saves
def test_a_forward_and_saves(R):
    c, n, K = R.c, R.n, R.c.K
    main = R.main
    ran = main["ran"]
    want_native = R.prec == "fp32h2" and c.used is not None
    assert (ran["native"], ran["python"]) == ((1, 0) if want_native else (0, 1)), ran
    # feat under the forward suite's two bars; rows without a neighbour stay zero
    ref, e, sc, _ = AR.ref64_and_noise(R.name, R.masked)
    feat = main["feat"]
    assert feat.shape == (c.n_max, 129)
    unt = ref["untouched"][:n]
    assert not feat[:n][unt].any(), "rows without a neighbour were written"
    wr = ~unt
    over = []
    for blk, sl in (("alpha", slice(0, 1)), ("colour", slice(1, 129))):
        w = ref["feat"][:n][wr][:, sl]
        if not w.size:
            continue
        dlt = np.abs(feat[:n][wr][:, sl].astype(np.float64) - w)
        bar = float((dlt / (AR.ATOL + AR.RTOL * np.abs(w))).max())
        noise = max(e[blk], AR.ULP_FLOOR * sc[blk])
        r = float(dlt.max()) / noise
        print(f"RATIO {R.path:7s} {R.name:18s} {'feat ' + blk:22s} err {dlt.max():.3e}  e_o32 {e[blk]:.3e}  "
              f"max|g64| {sc[blk]:.3e}  err/noise {r:8.3f}  err/bar {bar:.5f}")
        wst = WORST.setdefault((R.path, "feat " + blk), [-1.0, R.name])
        if r > wst[0]:
            wst[0], wst[1] = r, R.name
        if bar > 1.0 or r > AR.C_TIGHT:
            over.append((blk, bar, r))
    assert not over, f"{R.path} {R.name}: feat over the project bar or c = {AR.C_TIGHT}: {over}"
    if n == 0:
        return
    # the saves
    s = R.saves()
    r64, en, scn = R.ref()
    mask, idx = r64["mask"], r64["idx"]
    prow = np.full((n, 8), -1, np.int64)
    prow[:, :K] = np.where(mask, idx, -1)
    assert np.array_equal(s["prow"], prow)   # (pair tables: the pair's own row)
    assert np.array_equal(s["vmask"] != 0, mask.any(-1))
    live = prow >= 0
    assert not s["wt"][~live].any(), "wt of an empty pair is not 0"
    aux = r64["aux"]
    for k in ("wt", "wn"):
        _close(s[k][:, :K][mask], aux[k][mask], k, rel=1e-5, scale=1e-6)
    _close(s["x3e"][:, :K, :7][mask], aux["x3e"][mask], "x3e", rel=1e-5, scale=1e-6)
    _close(s["pe5"][:, :K, :60][mask], aux["pe5"][mask], "pe5", rel=0.0, scale=3e-5)
    # hid = the K-sum of wt h4 over the saved values: eight fp32 roundings of the terms
    terms = s["wt"].astype(np.float64)[..., None] * s["h4"].astype(np.float64)
    hid64, mag = terms.sum(1), np.abs(terms).sum(1)
    v = s["vmask"] != 0
    assert (np.abs(s["hid"][v] - hid64[v]) <= 2.0 ** -20 * mag[v] + 1e-37).all(), "hid is not the K-sum of wt h4"
    # the pinning condition: a saved sign differs from z64 > 0 only within fp32 noise of 0
    sg = R.signs()
    for k in TR.SIGN_KEYS:
        if k == "pa" and c.act_super:
            continue
        rows = mask if k in ("h1", "h2", "h3", "h4", "pa") else v
        z64 = r64["z"][k][rows]
        dis = sg[k][rows] != (z64 > 0)
        bar = TR.tight_bar(en["z:" + k], scn["z:" + k])
        print(f"SIGNS {R.path:7s} {R.name:18s} {k:4s} {int(dis.sum())} of {dis.size} differ from z64 > 0 (bar {bar:.2e})")
        assert not dis.any() or np.abs(z64[dis]).max() <= bar, \
            (R.path, R.name, k, int(dis.sum()), float(np.abs(z64[dis]).max()), bar)
    # the mask words against the saved post-activations (every slot of the rows < n)
    bits = _mask_bits(s["mask"])
    for li, k in enumerate(("h1", "h2", "h3", "h4")):
        pos = s[k] > 0
        if c.neg_slope > 0:
            assert np.array_equal(bits[:, :, li], pos), f"mask words of {k} differ from saved h > 0"
        else:
            assert not (bits[:, :, li] & ~pos).any(), f"mask bit of {k} set where saved h <= 0"


# ------------------------------------------------------------------ (b) the pairs chain
def test_b_pairs_chain(R):
    b = R.main["ran"]["stages"]
    if b is None or R.n == 0:   # the native step keeps no per-pair rows; an empty list has none
        return
    n, K = R.n, R.c.K
    mask = R.ref()[0]["mask"]
    empty = np.ones((n, 8), bool)
    empty[:, :K] = ~mask
    got = {f"dz{i + 1}": _np(b.dz[i][:n * 8]).reshape(n, 8, 256) for i in range(4)}
    got["dpa"] = _np(b.dpa[:n * 8]).reshape(n, 8)
    if b.dconf_pair is not None:
        got["dconf_pair"] = _np(b.dconf_pair[:n * 8]).reshape(n, 8)
    for k, g in got.items():
        assert not g[empty].any(), f"{k}: a row of an empty pair is not 0"
    R.check({k: (np.ascontiguousarray(g[:, :K]), k) for k, g in got.items()})


# ------------------------------------------------------------------ (c) point gradients
def _point_tensors(R, out):
    names = dict(emb="emb", color="color", dir="dir", conf="conf")
    return {"d " + k: (out["grads"][k].reshape(R.ref()[0]["grads"][key].shape), key)
            for k, key in names.items() if out["grads"][k] is not None}


def test_c_point_gradients(R):
    c = R.c
    main = R.main
    r64 = R.ref()[0]
    referenced = np.zeros(c.N, bool)
    if R.n:
        referenced[r64["idx"][r64["mask"]]] = True
    for k in ("emb", "color", "dir", "conf"):
        g = main["grads"][k]
        if g is not None:
            assert g.shape[0] == c.N and not g[~referenced].any(), f"d {k}: a row of an unreferenced point is not 0"
    R.check(_point_tensors(R, main))
    # two backward runs bitwise equal (no float atomics on the way to a point row)
    R._memo.pop((False, True))
    again = R.execute()
    for k in ("emb", "color", "dir", "conf"):
        if main["grads"][k] is not None:
            assert np.array_equal(main["grads"][k], again["grads"][k]), f"d {k}: two runs differ"
    if main["ran"]["native"]:   # the native step against the Python sequence of the same kernels
        seq = R.execute(native=False)
        assert (seq["ran"]["native"], seq["ran"]["python"]) == (0, 1)
        for k in ("emb", "color", "dir", "conf"):
            if main["grads"][k] is not None:
                assert np.array_equal(main["grads"][k], seq["grads"][k]), f"d {k}: native step != Python sequence"


# ------------------------------------------------------------------ (d) parameter gradients
def test_d_parameter_gradients(R):
    main = R.main
    R.check({"d " + k: (main["grads"][k], k) for k in TR.PARAM_NAMES})


# ------------------------------------------------------------------ (e) d xyz
def test_e_xyz_gradient(R):
    if not R.xyz_ok:   # pers given (pers_given, the pair-table twins): pers is not w2pers(xyz)
        return
    out = R.execute(xyz_grad=True)
    assert (out["ran"]["native"], out["ran"]["python"]) == (0, 1)
    assert np.array_equal(out["feat"][:R.n], R.main["feat"][:R.n])
    R.check({"d xyz": (out["grads"]["xyz"], "xyz")})


# ------------------------------------------------------------------ empty and degenerate lists
def test_empty_list_gives_zero_gradients(cuda):
    """ndev_0: *n_dev = 0 under n_max = 100 -- no launch error, every gradient exactly 0."""
    for prec in PRECISIONS:
        out = Run("ndev_0", prec, False, cuda).execute(xyz_grad=True)
        for k, g in out["grads"].items():
            assert g is not None and not g.any(), (prec, k)


@pytest.mark.parametrize("name, pairs", [("count_1", 4), ("ntail_1", 170)])
def test_degenerate_lists(cuda, name, pairs):
    """One sample; and a one-point table: the 170 filled slots of its 41 x 8 all reference
    point 0 (a group of more than 32: the workgroup path of pnr_group_pairs)."""
    c = AR.case(name)
    assert int((c.pidx >= 0).sum()) == pairs
    if name == "ntail_1":
        assert c.N == 1 and (c.pidx[c.pidx >= 0] == 0).all()
    for prec in PRECISIONS:
        run = Run(name, prec, False, cuda)
        assert all(np.isfinite(g).all() for g in run.main["grads"].values() if g is not None)
        run.check(_point_tensors(run, run.main))


# ------------------------------------------------------------------ pnr_group_pairs
GROUP_SIZES = (1, 31, 32, 33, 64, 65, 256, 257, 700, 5000)


def _group_keys(seed, sizes, n_keys, holes=0.1):
    """prow [m]: key q (spread over [0, n_keys)) sizes[q] times, interleaved in pair order
    by a seeded shuffle, about ``holes`` of the entries -1."""
    g = torch.Generator().manual_seed(seed)
    keys = torch.randperm(n_keys, generator=g)[:len(sizes)].int()
    prow = torch.cat([torch.full((L,), int(k), dtype=torch.int32) for k, L in zip(keys, sizes)])
    prow = torch.cat([prow, torch.full((int(holes * prow.numel() / (1 - holes)),), -1, dtype=torch.int32)])
    return prow[torch.randperm(prow.numel(), generator=g)]


def _check_grouping(prow, with_map, n_keys, cuda, scr):
    """One pnr_group_pairs call on the given scratch against torch.sort(stable=True)."""
    from pointnerf_amd import _lib as L
    used = torch.unique(prow[prow >= 0]).int()
    used_map = torch.full((n_keys,), -1, dtype=torch.int32)
    used_map[used.long()] = torch.arange(used.numel(), dtype=torch.int32)
    m = prow.numel()
    d, key_map = prow.to(cuda), (used_map.to(cuda) if with_map else None)
    ps, po = (torch.full((m,), -7, dtype=torch.int32, device=cuda) for _ in range(2))
    L.check(L.lib().pnr_group_pairs(L.ptr(d), m, L.ptr(key_map), used.numel() if with_map else n_keys, L.ptr(ps),
                                    L.ptr(po), L.ptr(scr), scr.numel(), L.stream_ptr(cuda)), "pnr_group_pairs")
    rs, ro = torch.sort(prow, stable=True)
    nv = int((prow >= 0).sum())
    assert torch.equal(ps.cpu()[:nv], rs[m - nv:]) and torch.equal(po.cpu()[:nv], ro[m - nv:].int())
    assert bool((ps.cpu()[nv:] == -1).all())


@pytest.mark.parametrize("with_map", [True, False])
def test_group_pairs_at_the_group_size_edges(cuda, with_map):
    """Group sizes on and next to the 32-entry edge between the per-thread and the workgroup
    sort, up to 5000: equal to torch.sort(stable=True) exactly; then a call of another size
    (keys of 1 .. 40 pairs) on the same scratch, left as the first call wrote it."""
    from pointnerf_amd import _lib as L
    first, second = _group_keys(3, GROUP_SIZES, 9000), _group_keys(4, (1, 2, 33, 40, 7, 32), 300)
    scr = L.scratch("pnr_group_pairs_scratch_bytes", first.numel(), 9000, device=cuda)
    _check_grouping(first, with_map, 9000, cuda, scr)
    _check_grouping(second, with_map, 300, cuda, scr)


def test_group_pairs_time_at_5000(cuda):
    """The quadratic rank of a 5000-pair group (a number to have, not a bar)."""
    from pointnerf_amd import _lib as L
    prow = _group_keys(3, GROUP_SIZES, 9000).to(cuda)
    L.group_pairs(prow, None, 9000)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(10):
        L.group_pairs(prow, None, 9000)
    ev[1].record()
    torch.cuda.synchronize()
    print(f"GROUP pnr_group_pairs, m = {prow.numel()}, largest group 5000: {ev[0].elapsed_time(ev[1]) / 10 * 1e3:.1f} us")


# ------------------------------------------------------------------ the atomic d_p1 form
@pytest.mark.parametrize("name", ["count_65", "used_subset"])
def test_bwd_pairs_atomic_d_p1(cuda, name):
    """pnr_aggregate_bwd_pairs with d_p1 given (float atomics into the point rows, used_map
    rows with a used subset) against pnr_pairs_to_points' result, within the tight bar
    (c = 8) of the float64 per-point sum."""
    from pointnerf_amd import _lib as L
    run = Run(name, "fp32", False, cuda)
    b = run.main["ran"]["stages"]
    c, n = run.c, run.n
    f32 = dict(dtype=torch.float32, device=cuda)
    Pn = n * 8
    dz = [torch.empty((Pn, 256), **f32) for _ in range(4)]
    dpa, dcp = torch.empty(Pn, **f32), torch.empty(Pn, **f32)
    d_p1 = torch.zeros((b.n_p1, 256), **f32)
    d_color, d_dir = torch.zeros((c.N, 3), **f32), torch.zeros((c.N, 3), **f32)
    L.check(L.lib().pnr_aggregate_bwd_pairs(*b._refs(), L.ctypes.byref(b.packs.mlp), L.ctypes.byref(b.sv.c),
                                            L.ptr(b.d_feat), L.ptr(b.d_hid), *(L.ptr(t) for t in dz), L.ptr(dpa),
                                            L.ptr(d_p1), L.ptr(d_color), L.ptr(d_dir), L.ptr(dcp),
                                            L.stream_ptr(cuda)), "pnr_aggregate_bwd_pairs")
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(dz[i], b.dz[i][:Pn])
    r64, e, sc = run.ref()
    want = r64["grads"]["d_p1"]
    rows = np.arange(c.N) if c.used is None else c.used[:run.main["n_used"]]
    want = want[rows]
    bar = TR.tight_bar(e["d_p1"], sc["d_p1"], 8.0)
    ref_rows = np.abs(want).max(1) > 0           # pnr_pairs_to_points writes the referenced rows only
    for nm, got in (("atomic", _np(d_p1)), ("pairs_to_points", _np(b.d_p1))):
        err = float(np.abs(got[:rows.size][ref_rows] - want[ref_rows]).max())
        print(f"RATIO fp32    {name:18s} {'d_p1 ' + nm:22s} err {err:.3e}  e_o32 {e['d_p1']:.3e}  "
              f"max|g64| {sc['d_p1']:.3e}  err/noise {err / (bar / 8.0):8.3f}")
        assert err <= bar, (nm, err, bar)
    assert not _np(d_p1)[:rows.size][~ref_rows].any()
