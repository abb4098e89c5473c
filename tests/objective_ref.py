"""TEST INFRASTRUCTURE ONLY -- cases and float64 / float32 restatements for the
finetune step's leaf kernels outside the aggregate, called directly:

  A  pnr_sparse_loss_fwd / _bwd (loss.hip) on composite_ref.make_bufs' query buffers;
  B  pnr_point_counts (aggregate_points.hip) and pnr_zero_one_loss_fwd / _bwd
     (composite.hip) on hand-built neighbour lists, counts and conf tables;
  C  pnr_rgb_head_fwd / _bwd (head.hip);
  (D, pnr_adam_step across launches, lives in tests/test_gpu_optim.py).

The cases live here so that the CPU test (tests/test_objective_ref_host.py) can show,
for every one of them, that correct fp32 arithmetic -- the restatement itself, or an
emulation of the kernel's own summation order -- meets the bar the GPU test
(tests/test_gpu_objective.py) asks of the kernels.

Bars (none of them measured from the kernels):
  * sparse loss and zero-one loss, values and d_conf: loss_ref.within -- at most
    4 x the fp32 restatement's own error against float64 plus one fp32 ulp of the
    tensor's largest entry;
  * w_fix: integer equality with sum rint(float64(w) 2^38) over pnr_march_aux's own
    fp32 weights, and |w_fix / 2^38 - W64| <= sum over the point's pairs of
    (2e-5 max|w64| + 1e-4 w64 + 2^-39): pnr_march_aux's bar per weight
    (composite_ref.SCALE / REL) plus half a quantisation step;
  * point counts: exact;
  * rgb head, per tensor: max|got - ref64| <= C_TIGHT max(e_o32, 2^-22 max|ref64|),
    e_o32 = the numpy fp32 restatement against float64 on the same case.
"""
from __future__ import annotations

import numpy as np
import torch

import aggregate_ref as AR
import composite_ref as CR
import loss_ref as LR

F32 = np.float32
C_TIGHT = AR.C_TIGHT
ULP_FLOOR = AR.ULP_FLOOR
W_SCALE = 2.0 ** 38          # kWScale of loss.hip
SPARSE_MAX_PAIRS = 1 << 25   # kSparseMaxPairs
LOSS_BLOCKS = 256            # kLossBlocks
ZO_BLOCKS = 512              # kZoBlocks
HEAD_BWD_BLOCKS = 512        # PNR_HEAD_BWD_BLOCKS
UP_SPARSE = 0.37             # upstream gradient of the sparse loss
UP_ZO = 1e-4                 # upstream gradient of the zero-one loss (its shipped weight)


# ============================================================== A. sparse loss
# name -> (SR, K, N, conf pattern, variant).  Every SR, K and N of the issue appears;
# (128, 16) with N = 1: every pair gathers the one point.
SPARSE_CASES = {
    "sr1_k1_n37": (1, 1, 37, "uniform", None),
    "sr63_k3_n255": (63, 3, 255, "uniform", None),
    "sr64_k8_n256_low": (64, 8, 256, "low", None),
    "sr65_k8_n257": (65, 8, 257, "uniform", None),
    "sr80_k8_n513_high": (80, 8, 513, "high", None),
    "sr128_k16_n1": (128, 16, 1, "uniform", None),
    "sr128_k16_n5000": (128, 16, 5000, "uniform", None),
    "sr63_k3_n1_low": (63, 3, 1, "low", None),
    "sr65_k8_n5000_null": (65, 8, 5000, "null", None),
    "sr128_k16_n1_null": (128, 16, 1, "null", None),
    "sr80_k8_n256_high": (80, 8, 256, "high", None),
    "sr64_k8_n37_R0": (64, 8, 37, "uniform", "R0"),
    "sr80_k8_n257_novalid": (80, 8, 257, "uniform", "novalid"),
    "sr65_k8_n200_oob": (65, 8, 200, "uniform", "oob"),
}
OOB_EXTRA = 100   # the "oob" buffers index N + OOB_EXTRA points; the call is told N


def sparse_case(name):
    """dict: bufs (what the kernel gets), ref_bufs (what the expected values are
    computed from), N, R, conf [N] float32 or None, name."""
    SR, K, N, pat, variant = SPARSE_CASES[name]
    seed = sorted(SPARSE_CASES).index(name)
    R = 0 if variant == "R0" else CR.FUSED_R
    n_points = N + OOB_EXTRA if variant == "oob" else N
    b = CR.make_bufs(R, SR, K=K, seed=seed, n_points=n_points)
    ref = b
    if variant == "novalid":
        b = dict(b, ray_vcnt=torch.zeros_like(b["ray_vcnt"]), ray_row=torch.zeros_like(b["ray_row"]), R_valid=0)
        ref = b
    if variant == "oob":
        p = b["pidx"].clone()
        assert int((p >= N).sum()) > 0
        p[p >= N] = -1
        ref = dict(b, pidx=p)
    rng = np.random.default_rng(9100 + seed)
    conf = {"uniform": lambda: rng.uniform(-0.1, 1.1, N), "low": lambda: rng.uniform(-0.1, 9e-5, N),
            "high": lambda: rng.uniform(1.0001, 1.5, N), "null": lambda: None}[pat]()
    return dict(name=name, bufs=b, ref_bufs=ref, N=N, R=R, SR=SR, K=K,
                conf=None if conf is None else conf.astype(F32))


def dense_pidx(bufs):
    """pidx in pnr_march_aux's weight layout, [R'',SR,K] int64: rows in ray_row order
    of the rays with ray_vcnt > 0, -1 in the slots at or past n_filled."""
    out = torch.full((bufs["R_valid"], bufs["SR"], bufs["K"]), -1, dtype=torch.long)
    for r in range(bufs["R"]):
        if bufs["ray_vcnt"][r] <= 0:
            continue
        row, n, off = int(bufs["ray_row"][r]), int(bufs["n_filled"][r]), int(bufs["ray_off"][r])
        out[row, :n] = bufs["pidx"][off:off + n].long()
    return out


def sparse_reference(c, dtype):
    """loss_ref.sparse_item on composite_ref.aux_weight_reference(dtype) with the
    straight-through clamp of the gathered conf -> dict loss (0-d), d_conf [N] (for
    the upstream gradient UP_SPARSE; zeros without a conf table), W [N] (the summed
    weight per point), w [R'',SR,K], pairs [N] (how many pairs gather each point)."""
    b, N = c["ref_bufs"], c["N"]
    w = CR.aux_weight_reference(b, dtype)
    pd = dense_pidx(b)
    d = torch.zeros(N, dtype=dtype)
    if c["conf"] is None:
        cc, leaf = torch.ones((), dtype=dtype), None
    else:
        leaf = torch.from_numpy(c["conf"]).to(dtype).requires_grad_(True)
        cf = leaf[pd.clamp(min=0)]
        cc = cf - (cf - torch.clamp(cf, 1e-4, 1.0)).detach()
    loss = LR.sparse_item(w, cc)
    if leaf is not None:
        (loss * UP_SPARSE).backward()
        if leaf.grad is not None:
            d = leaf.grad.detach()
    flat, sel = pd.reshape(-1), (pd >= 0).reshape(-1)
    W = torch.zeros(N, dtype=dtype).index_add_(0, flat[sel], w.detach().reshape(-1)[sel])
    pairs = torch.zeros(N, dtype=torch.long).index_add_(0, flat[sel], torch.ones(int(sel.sum()), dtype=torch.long))
    return dict(loss=loss.detach(), d_conf=d, W=W, w=w.detach(), pairs=pairs)


def wfix_from_weights(w32, bufs, N):
    """sum rint(float64(w) 2^38) per point over the pairs of [R'',SR,K] fp32 weights
    (numpy), int64 [N]: what k_sparse_weights must leave in w_fix when its weights
    are pnr_march_aux's, term by term."""
    pd = dense_pidx(bufs).numpy().reshape(-1)
    q = np.rint(np.asarray(w32, F32).astype(np.float64).reshape(-1) * W_SCALE).astype(np.int64)
    sel = pd >= 0
    out = np.zeros(N, np.int64)
    np.add.at(out, pd[sel], q[sel])
    return out


def wfix_bar(ref64):
    """check 2's allowance per point, float64 [N]."""
    w, W, pairs = ref64["w"].numpy(), ref64["W"].numpy(), ref64["pairs"].numpy()
    wmax = float(np.abs(w).max()) if w.size else 0.0
    return pairs * (CR.SCALE * wmax + 2.0 ** -39) + CR.REL * W


def sparse_from_wfix(wfix, conf, g=UP_SPARSE):
    """k_sparse_part / _final / _bwd from a w_fix table, as the kernels state them:
    float64 sums rounded to fp32 once -> (loss fp32, d_conf [N] fp32, den)."""
    q = np.asarray(wfix, np.int64).astype(np.float64)
    cc = np.ones(q.shape) if conf is None else np.clip(np.asarray(conf, F32), F32(1e-4), F32(1)).astype(np.float64)
    e = np.exp(-2.0 * cc)
    den = float(np.asarray(wfix, np.int64).sum()) / W_SCALE + 1e-6
    loss = F32((q * np.abs(1.0 - e)).sum() / W_SCALE / den)
    d = (g / (den * W_SCALE) * q * np.sign(1.0 - e) * 2.0 * e).astype(F32)
    return loss, d, den


# ================================================ B. point counts and zero-one loss
COUNT_CASES = {1: (300, 97), 8: (301, 61), 16: (64, 5)}   # K -> (S rows, points)


def count_case(K):
    S, N = COUNT_CASES[K]
    rng = np.random.default_rng(500 + K)
    pidx = rng.integers(0, N, (S, K)).astype(np.int32)
    pidx[rng.random((S, K)) < 0.3] = -1
    pidx[S // 3] = -1                      # a whole row without a neighbour
    prefill = rng.integers(0, 5, N).astype(F32)
    return dict(K=K, S=S, N=N, pidx=pidx, prefill=prefill, n_dev=(0, 1, S // 2, S, S + 5, -3))


def count_reference(c, n):
    """prefill + bincount over the first min(max(n, 0), S) rows, float32 [N]."""
    rows = min(max(int(n), 0), c["S"])
    flat = c["pidx"][:rows].reshape(-1)
    return c["prefill"] + np.bincount(flat[flat >= 0], minlength=c["N"]).astype(F32)


# name -> (N, eps, point 0 has a count of its own, empty entries)
ZO_CASES = {
    "n1_e7": (1, 1e-3, False, 7),
    "n1_own": (1, 1e-2, True, 0),
    "n511_own": (511, 1e-3, True, 0),
    "n512_e7": (512, 1e-2, False, 7),
    "n513_own_e3000": (513, 1e-3, True, 3000),
    "n513_p0_nothing": (513, 1e-2, False, 0),
    "n5000_e4000": (5000, 1e-2, False, 4000),
    "n5000_own_e7": (5000, 1e-3, True, 7),
    "n512_rvalid0": (512, 1e-3, False, 0),
    "n8_big": (8, 1e-3, True, None),
}


def zo_bounds(eps):
    """(eps, 1 - eps) as the kernel compares them: fp32, the upper one subtracted in fp32."""
    e = F32(eps)
    return e, F32(1) - e


def zo_planted(eps):
    """The clamp edges and their fp32 neighbours, 0, a negative value, a value above 1."""
    lo, hi = zo_bounds(eps)
    out = []
    for b in (F32(1e-4), lo, hi, F32(1)):
        out += [b, np.nextafter(b, F32(-np.inf)), np.nextafter(b, F32(np.inf))]
    return np.array(out + [F32(0), F32(-0.05), F32(1.07)], F32)


def zo_case(name):
    """dict conf [N] f32, counts [N] f32 (integers), r_valid, srk, eps, E, empty."""
    N, eps, own, empty = ZO_CASES[name]
    rng = np.random.default_rng(600 + sorted(ZO_CASES).index(name))
    lo, hi = zo_bounds(eps)
    if name == "n8_big":
        conf = np.array([0.3, lo, hi, np.nextafter(hi, F32(np.inf)), 1e-4, 0.7, np.nextafter(lo, F32(-np.inf)), 0.5], F32)
        counts = (3_000_000 + np.array([-1, 1, 3, 5, 7, 9, 11, 14])).astype(F32)   # an odd total above 2^24: no fp32 number
        r_valid, srk = 24576, 1024
    else:
        conf = rng.uniform(-0.1, 1.1, N).astype(F32)
        conf[0] = F32(rng.uniform(0.05, 0.95))
        counts = rng.integers(1, 40, N).astype(np.int64)
        counts[rng.random(N) < 0.2] = 0
        if N >= 32:
            pl = zo_planted(eps)
            conf[1:1 + pl.size] = pl
            counts[1:1 + pl.size] = np.maximum(counts[1:1 + pl.size], 1)
        elif name == "n1_own":
            conf[0] = lo                          # exactly eps: inside the inclusive mask
        counts[0] = 13 if own else 0
        if name == "n512_rvalid0":
            counts[:] = 0
            r_valid, srk = 0, 4
        else:
            srk = 1 if N == 1 else 4
            if srk > 1:
                counts[N - 1] += (-(int(counts.sum()) + empty)) % srk
            r_valid = (int(counts.sum()) + empty) // srk
        counts = counts.astype(F32)
    E = r_valid * srk
    c = dict(name=name, N=N, eps=eps, conf=conf, counts=counts, r_valid=r_valid, srk=srk, E=E,
             empty=E - int(counts.astype(np.int64).sum()))
    assert c["empty"] >= 0 and (empty is None or c["empty"] == empty or name == "n512_rvalid0")
    return c


def _zo_terms(c, dt):
    lo, hi = zo_bounds(c["eps"])
    cc = np.clip(c["conf"], F32(1e-4), F32(1))
    v = np.clip(cc, lo, hi).astype(dt)
    mask = (cc >= lo) & (cc <= hi)            # torch.clamp's gradient mask, inclusive
    with np.errstate(divide="ignore"):
        f = np.log(v) + np.log(dt(1) - v)
        df = dt(1) / v - dt(1) / (dt(1) - v)
    return f, df, mask


def zo_truth(c):
    """(loss, d_conf [N]) in float64 from the fp32 inputs: (sum c_p f(v_p) + empty
    f(v_0)) / E and c_p g / E f'(v_p) under the inclusive mask, point 0 carrying the
    empty entries; all 0 for E = 0."""
    f, df, mask = _zo_terms(c, np.float64)
    cnt = c["counts"].astype(np.float64)
    if c["E"] == 0:
        return np.float64(0), np.zeros(c["N"])
    loss = (float((cnt * f).sum()) + c["empty"] * float(f[0])) / c["E"]
    ct = cnt.copy()
    ct[0] += c["empty"]
    d = np.where(mask & (ct != 0), ct * float(F32(UP_ZO)) / c["E"] * df, 0.0)
    return np.float64(loss), d


def zo_yardstick(c):
    """The same in float32: loss_ref.zero_one_item on the expanded gathered tensor by
    torch autograd; above 2e6 entries the count-weighted form in fp32 numpy."""
    if c["E"] == 0:
        return F32(0), np.zeros(c["N"], F32)
    if c["E"] > 2e6:
        f, df, mask = _zo_terms(c, F32)
        ct = c["counts"].copy()
        E = F32(c["E"])
        loss = (np.sum(ct * f, dtype=F32) + F32(c["empty"]) * f[0]) / E
        ct[0] += F32(c["empty"])
        return F32(loss), np.where(mask & (ct != 0), ct * F32(UP_ZO) / E * df, F32(0)).astype(F32)
    leaf = torch.from_numpy(c["conf"].copy()).requires_grad_(True)
    idx = torch.cat([torch.repeat_interleave(torch.arange(c["N"]), torch.from_numpy(c["counts"]).long()),
                     torch.zeros(c["empty"], dtype=torch.long)])
    cf = leaf[idx]
    cc = cf - (cf - torch.clamp(cf, 1e-4, 1.0)).detach()
    loss = LR.zero_one_item(cc, c["eps"])
    (loss * UP_ZO).backward()
    return F32(float(loss.detach())), leaf.grad.numpy()


def _butterfly(a):
    """The xor-shuffle sum of 64 lanes (offsets 32 .. 1) along the last axis, fp32."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = (a + a[..., lanes ^ o]).astype(F32)
    return a[..., 0]


def zo_emulate(c):
    """k_zero_one_part / _final / _bwd in fp32 numpy, in the kernels' summation order
    -> (out [3], d_conf [N])."""
    N = c["N"]
    f, df, mask = _zo_terms(c, F32)
    cnt = c["counts"]
    per = -(-N // ZO_BLOCKS)
    s1 = np.zeros((ZO_BLOCKS, 256), F32)
    s0 = np.zeros((ZO_BLOCKS, 256), F32)
    b0 = (np.arange(ZO_BLOCKS) * per)[:, None]
    b1 = np.minimum(b0 + per, N)
    for j in range(-(-per // 256)):
        p = b0 + np.arange(256)[None, :] + 256 * j
        ok = p < b1
        pc = np.where(ok, p, 0)
        use = ok & (cnt[pc] != 0)
        s1 = np.where(use, s1 + cnt[pc] * f[pc], s1).astype(F32)
        s0 = np.where(use, s0 + cnt[pc], s0).astype(F32)
    part = []
    for s in (s1, s0):
        w = _butterfly(s.reshape(ZO_BLOCKS, 4, 64))
        part.append((((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32))
    tot = []
    for p in part:
        t = np.zeros(64, F32)
        for i in range(ZO_BLOCKS // 64):
            t = (t + p[64 * i:64 * (i + 1)]).astype(F32)
        tot.append(_butterfly(t))
    E = F32(float(c["r_valid"]) * float(c["srk"]))
    empty = F32(E - tot[1])
    out = np.array([(tot[0] + empty * f[0]) / E if E > 0 else 0, empty, E], F32)
    scale = F32(UP_ZO) / E if E > 0 else F32(0)
    ct = cnt.copy()
    ct[0] = F32(ct[0] + empty)
    d = np.where(mask & (ct != 0), (ct * scale).astype(F32) * df, F32(0)).astype(F32)
    return out, d


def zo_must_be_zero(c):
    """Entries whose reference gradient is exactly 0: masked, or without a count."""
    return zo_truth(c)[1] == 0


# ================================================================== C. rgb head
# name -> (n_max, n_dev kind, ld, act_super, weight scale, saturated rows planted)
HEAD_CASES = {
    "n0_null": (0, "null", 129, 1, 0.1, False),
    "n0_eq": (0, "eq", 136, 0, 1.0, False),
    "n1_eq": (1, "eq", 136, 0, 1.0, False),
    "n7_m9": (7, "m9", 129, 1, 1.0, False),
    "n7_zero": (7, "zero", 129, 0, 0.1, False),
    "n8_p5": (8, "p5", 136, 1, 0.1, False),
    "n9_null": (9, "null", 136, 0, 0.1, False),
    "n9_m9": (9, "m9", 129, 1, 1.0, False),
    "n4095_m9": (4095, "m9", 129, 1, 1.0, False),
    "n4096_eq": (4096, "eq", 136, 0, 0.1, False),
    "n4097_null": (4097, "null", 129, 1, 0.1, False),
    "n4097_zero": (4097, "zero", 136, 1, 1.0, False),
    "n16400_m9": (16400, "m9", 136, 1, 0.1, False),
    "n16400_null": (16400, "null", 129, 0, 1.0, False),
    "n16400_p5": (16400, "p5", 129, 1, 1.0, False),
    "n4097_sat_super": (4097, "eq", 136, 1, 1.0, True),
    "n4097_sat_plain": (4097, "m9", 129, 0, 1.0, True),
}
SAT_SIGNS = ((1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1))
SAT_LOGIT = 120.0


def head_case(name):
    """dict feat [max(n_max, 1), ld], w [3,128], b [3], d_out [max(n_max, 1), 4]
    (fp32 numpy), n_dev (None or int), n (the rows the kernels touch), sat (rows whose
    three logits are +-SAT_LOGIT -> their signs)."""
    n_max, kind, ld, act, scale, sat = HEAD_CASES[name]
    rng = np.random.default_rng(700 + sorted(HEAD_CASES).index(name))
    rows = max(n_max, 1)
    feat = rng.standard_normal((rows, ld)).astype(F32)
    feat[:, 129:] = F32(1e3)                  # the pad columns: never read
    w = (rng.standard_normal((3, 128)) * scale).astype(F32)
    b = (rng.standard_normal(3) * scale).astype(F32)
    d_out = rng.standard_normal((rows, 4)).astype(F32)
    n_dev = {"null": None, "eq": n_max, "m9": max(n_max - 9, 0), "p5": n_max + 5, "zero": 0}[kind]
    n = n_max if n_dev is None else min(max(n_dev, 0), n_max)
    sat_rows = {}
    if sat:
        w64 = w.astype(np.float64)
        for i, sg in enumerate(SAT_SIGNS):
            for r in (i, n // 2 + i, n - 1 - i):      # first rows, the middle, the last rows
                a = np.linalg.solve(w64 @ w64.T, SAT_LOGIT * np.array(sg, np.float64) - b)
                feat[r, 1:129] = (a @ w64).astype(F32)
                sat_rows[r] = sg
    return dict(name=name, n_max=n_max, ld=ld, act=act, feat=feat, w=w, b=b, d_out=d_out, n_dev=n_dev, n=n,
                sat=sat_rows)


def head_reference(c, dt):
    """out [n,4], d_feat [n,129], dW [3,128], db [3] in numpy dtype dt."""
    n = c["n"]
    x = c["feat"][:n, 1:129].astype(dt)
    w, b, do = c["w"].astype(dt), c["b"].astype(dt), c["d_out"][:n].astype(dt)
    with np.errstate(over="ignore"):
        s = dt(1) / (dt(1) + np.exp(-(x @ w.T + b)))
    sc = dt(1) + dt(2e-3) if c["act"] > 0 else dt(1)
    out = np.concatenate([c["feat"][:n, :1].astype(dt), s * sc - dt(1e-3) if c["act"] > 0 else s], 1)
    g = do[:, 1:] * sc * s * (dt(1) - s)
    d_feat = np.concatenate([do[:, :1], g @ w], 1)
    return dict(out=out.astype(dt), d_feat=d_feat.astype(dt), dW=(g.T @ x).astype(dt), db=g.sum(0).astype(dt))


HEAD_TENSORS = ("out", "d_feat", "dW", "db")


def head_noise(c):
    """(ref64, e_o32 per tensor, max|ref64| per tensor)."""
    r64, r32 = head_reference(c, np.float64), head_reference(c, F32)
    e = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) if r64[k].size else 0.0 for k in HEAD_TENSORS}
    sc = {k: float(np.abs(r64[k]).max()) if r64[k].size else 0.0 for k in HEAD_TENSORS}
    return r64, e, sc


def head_ratio(got, ref64, e_o32, scale):
    """err / max(e_o32, 2^-22 max|ref64|); 0 for an empty tensor, inf for a non-finite one."""
    if ref64.size == 0:
        return 0.0, 0.0
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    noise = max(e_o32, ULP_FLOOR * scale)
    return err, (err / noise if noise > 0 else (0.0 if err == 0 else float("inf")))


def head_end_values(act):
    """(low, high) fp32 outputs of a saturated logit: sigmoid exactly 0 / 1."""
    if act > 0:
        return -F32(1e-3), F32(1) * (F32(1) + F32(2e-3)) - F32(1e-3)
    return F32(0), F32(1)
