"""TEST INFRASTRUCTURE ONLY -- numpy restatement of PointAggregator.forward's
``viewmlp`` (point_aggregators.py:488-646, 729-816) for ANY embedding width E and
agg_intrp_order 1 or 2, in a chosen dtype, and hand-built sample lists over wide
point tables for tests/test_gpu_aggregate_dtu.py.

``aggregate`` follows oracle.aggregate operation by operation (at E = 32, order 2
and the same dtype the two agree bit for bit: test_aggregate_dtu_host.py), with
the reference's input order for a wide table (networks.py:175-190: embedding rows
0..E-1, PE row E + 6c + {s0,c0,s1,c1,s2,c2} of channel c, then the 60 distance
columns from 7E) and order 1's tail (point_aggregators.py:573-599: alpha from the
K-summed block3 features, raw2out_color on the colour branch).  ``mut`` emulates
one plausible kernel bug of the wide per-point pass or the tail.

The cases reuse tests/aggregate_ref.py's generator; ``wide`` swaps the 32-wide
table for an E-wide one.  Bars as there: the project bar |d| <= 1e-4 + 1e-4 |ref64|
and the tight bar err <= C_TIGHT max(e_o32, 2^-22 max|ref64|), e_o32 = this
restatement's own fp32 error against fp64 on the case.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import aggregate_ref as AR
from formula import LEGO_SHAPES, formula_params
from oracle import oracle as O

MUTATIONS = ("pe_stride32", "split_224", "drop_ch62", "alpha_per_pair", "no_raw2out_color")
C_TIGHT = AR.C_TIGHT


def shapes_of(E):
    return dict(LEGO_SHAPES, **{"block1.0": (256, 7 * E + 60)})


def params_for(E, salt=0.0):
    """formula_params with block1.0 shaped (256, 7E + 60)."""
    return formula_params(shapes_of(E), salt=salt)


def _pe(x, freqs, F, ori=False):
    """oracle.positional_encoding in dtype F."""
    x = np.asarray(x, F)
    bands = (2.0 ** np.arange(freqs)).astype(F)
    pts = (x[..., None] * bands).reshape(x.shape[:-1] + (freqs * x.shape[-1],)).astype(F)
    if ori:
        return np.concatenate([x, np.sin(pts), np.cos(pts)], axis=-1).astype(F)
    return np.stack([np.sin(pts), np.cos(pts)], axis=-1).reshape(pts.shape[:-1] + (pts.shape[-1] * 2,)).astype(F)


def aggregate(params, sampled_color, sampled_Rw2c, sampled_dir, sampled_conf, sampled_embedding,
              sampled_xyz_pers, sampled_xyz, sample_pnt_mask, sample_loc, sample_loc_w, sample_ray_dirs,
              neg_slope=0.01, act_super=1, order=2, dtype=np.float32, mut=None):
    """Inputs [R,SR,K,.] (B = 1 dropped) -> features [R,SR,129], ray_valid [R,SR], weight, conf_coefficient
    [R,SR,K], all in ``dtype``; E = sampled_embedding.shape[-1]."""
    assert order in (1, 2) and (mut is None or mut in MUTATIONS)
    F, C = dtype, 128
    E = np.asarray(sampled_embedding).shape[-1]

    def lin(x, name, W=None):
        W = np.asarray(params[name + ".weight"], F) if W is None else W
        b = np.asarray(params[name + ".bias"], F)
        return (np.matmul(x.astype(F), W.T).astype(F) + b).astype(F)

    def lrelu(x):
        return np.where(x > 0, x, x * F(neg_slope)).astype(F)

    def softplus(x):
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20)))).astype(F)

    mask = np.asarray(sample_pnt_mask, bool)
    R, SR, K = mask.shape
    ray_valid = mask.any(-1)
    sx, sxp = np.asarray(sampled_xyz, F), np.asarray(sampled_xyz_pers, F)
    sl, slw = np.asarray(sample_loc, F), np.asarray(sample_loc_w, F)
    xdist = (sxp[..., 0] * sxp[..., 2]).astype(F) - (sl[:, :, None, 0] * sl[:, :, None, 2]).astype(F)
    ydist = (sxp[..., 1] * sxp[..., 2]).astype(F) - (sl[:, :, None, 1] * sl[:, :, None, 2]).astype(F)
    zdist = sxp[..., 2] - sl[:, :, None, 2]
    dists = np.concatenate([(sx - slw[..., None, :]).astype(F),
                            np.stack([xdist, ydist, zdist], -1).astype(F)], -1).astype(F)
    w = (1.0 / np.maximum(np.sqrt((dists[..., :3] ** 2).sum(-1)), F(1e-6))).astype(F)
    w = (mask * w).astype(F)
    w = (w / np.maximum(w.sum(-1, keepdims=True), F(1e-8))).astype(F)
    conf = np.ones(mask.shape, F) if sampled_conf is None else np.asarray(sampled_conf, F)[..., 0]
    confc = np.clip(conf, F(1e-4), F(1)).astype(F)
    wt = (w * confc).astype(F)
    Rw = np.eye(3, dtype=F) if sampled_Rw2c is None else np.asarray(sampled_Rw2c, F)
    per_pair = Rw.ndim > 2

    def rot(x, Rm):
        if Rm.ndim == 2:
            return (x @ Rm.T).astype(F)
        return np.einsum("ni,nji->nj", x, Rm).astype(F)

    out = np.zeros((R, SR, C + 1), F)
    if not ray_valid.any():
        return out, ray_valid, w, confc
    pm = mask.reshape(-1)
    Rpair = Rw.reshape(-1, 3, 3)[pm] if per_pair else Rw
    Rray = Rw[:, :, 0].reshape(-1, 3, 3) if per_pair else Rw
    vd = rot(np.asarray(sample_ray_dirs, F).reshape(-1, 3), Rray)
    vpe = _pe(vd, 4, F, ori=True)
    ori_v, vpe = vpe[:, :3], vpe[:, 3:]
    vpe = vpe[ray_valid.reshape(-1)]
    d = dists.reshape(-1, 6)[pm].copy()
    d[:, :3] = rot(d[:, :3], Rpair)
    d = _pe(d, 5, F)
    e = np.asarray(sampled_embedding, F).reshape(-1, E)[pm]
    x1 = np.concatenate([e, _pe(e, 3, F)], -1)            # [., 7E]: the per-point half's inputs
    W1 = None
    if mut == "pe_stride32":      # PE of channel c written from row 32 + 6c, not E + 6c
        pe = x1[:, E:].reshape(-1, E, 6)
        for c in range(E):
            lo = 32 + 6 * c
            n = max(0, min(6, 7 * E - lo))
            x1[:, lo:lo + n] = pe[:, c, :n]
    elif mut == "drop_ch62" and E > 62:   # the channel loop stops at 62: its rows stay zero
        x1[:, 62] = 0
        x1[:, E + 6 * 62:E + 6 * 63] = 0
    feat = np.concatenate([x1, d], -1)
    if mut == "split_224":        # block1.0 cut at column 224: 224 point inputs, the distance half from 224
        W1 = np.asarray(params["block1.0.weight"], F)[:, :284]
        feat = np.concatenate([x1[:, :224], d], -1)
    feat = lrelu(lin(feat, "block1.0", W1))
    feat = lrelu(lin(feat, "block1.2"))
    col = np.asarray(sampled_color, F).reshape(-1, 3)[pm]
    sdir = rot(np.asarray(sampled_dir, F).reshape(-1, 3)[pm], Rpair)
    ov = np.repeat(ori_v[:, None, :], K, 1).reshape(-1, 3)[pm]
    feat = np.concatenate([feat, col, sdir - ov, (sdir * ov).sum(-1, keepdims=True)], -1).astype(F)
    feat = lrelu(lin(feat, "block3.0"))
    feat = lrelu(lin(feat, "block3.2"))

    def density(a):
        return softplus(a - 1) if act_super else np.maximum(a, 0)

    wv = wt.reshape(R * SR, K, 1)
    rvf = ray_valid.reshape(-1)
    fh = np.zeros((R * SR * K, feat.shape[-1]), F)
    fh[pm] = feat
    f = (fh.reshape(R * SR, K, -1) * wv).sum(-2)[rvf].astype(F)
    if order == 2 or mut == "alpha_per_pair":
        ah = np.zeros((R * SR * K, 1), F)
        ah[pm] = density(lin(feat, "alpha_branch.0"))
        alpha = (ah.reshape(R * SR, K, 1) * wv).sum(-2)[rvf]
    else:
        alpha = density(lin(f, "alpha_branch.0"))
    c = np.concatenate([f, vpe], -1)
    for name in ("color_branch.0", "color_branch.2", "color_branch.4"):
        c = lrelu(lin(c, name))
    if order == 1 and mut != "no_raw2out_color":          # raw2out_color (point_aggregators.py:269-273)
        c = (F(1) / (F(1) + np.exp(-c))).astype(F)
        if act_super > 0:
            c = (c * F(1 + 2 * 0.001) - F(0.001)).astype(F)
    flat = out.reshape(-1, C + 1)
    flat[rvf] = np.concatenate([alpha, c], -1)
    return out, ray_valid, w, confc


# ------------------------------------------------------------------ hand-built cases
def wide(c, E, order, seed):
    """The aggregate_ref case ``c`` with an E-wide embedding table and the order."""
    rng = np.random.default_rng(seed)
    w = SimpleNamespace(**vars(c))
    w.name = f"{c.name}/E{E}o{order}"
    w.emb = rng.uniform(-1.0, 1.0, (c.N, E)).astype(np.float32)
    w.E, w.order = E, order
    return w


def _geom(seed, **kw):
    return AR._geometry(AR.make_case("geom", seed, rows=19, **kw))


def _builders():
    b = {}
    # point counts on the 32- and 64-point tile edges of the two per-point kernels; every point referenced
    for i, n in enumerate((1, 31, 32, 33, 63, 64, 65, 257)):
        rows = 41 if n < 257 else 200
        b[f"n{n}"] = functools.partial(AR.make_case, f"n{n}", 2100 + i, rows=rows, N=n, cover_points=True,
                                       conf="out" if n in (33, 257) else "in")
    b["geom"] = functools.partial(_geom, 2200)                         # a point exactly at its sample
    b["conf_out"] = functools.partial(AR.make_case, "conf_out", 2201, rows=33, conf="out")
    b["used"] = lambda: AR._used_subset(AR.make_case("used", 2202, rows=37, N=1024), spare=40, device_count=True)
    b["relu"] = functools.partial(AR.make_case, "relu", 2203, rows=33, neg_slope=0.0, act_super=0,
                                  weights=("formula", 3.0))
    b["ndev"] = functools.partial(AR.make_case, "ndev", 2204, rows=100, n_max=100, n_dev=37)
    return b


_BUILDERS = _builders()
BASES = tuple(_BUILDERS)
# (base, E): 63 on every case, 64 and 33 on two each (a hard-coded 63; an aligned fast path)
WIDTHS = tuple((b, 63) for b in BASES) + (("n65", 64), ("geom", 64), ("n33", 33), ("used", 33))
CASES = tuple((b, E, o) for b, E in WIDTHS for o in (2, 1))
MASKED_OK = tuple(b for b in BASES if b != "used")


@functools.lru_cache(maxsize=None)
def case(base, E, order):
    c = wide(_BUILDERS[base](), E, order, seed=3000 + 7 * E + BASES.index(base))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case_params(c):
    kind, salt = c.weights
    assert kind == "formula"
    return params_for(c.E, salt)


def reference(c, dtype=np.float64, mut=None):
    """aggregate_ref.reference for a wide case: the restated gather, then ``aggregate`` above.
    -> dict(feat [n_max,129], untouched [n_max], rows, weight / conf [n_eff,K])."""
    K = c.K
    n_eff = max(0, min(int(c.n_dev), int(c.n_max)))
    feat = np.zeros((c.n_max, 129), dtype)
    untouched = np.ones(c.n_max, bool)
    v = np.arange(n_eff)
    rows = (c.samp_list[v] if c.samp_list is not None else v).astype(np.int64)
    if c.pidx is not None:
        pid = c.pidx[rows]
        mask = pid >= 0
        idx = np.maximum(pid, 0).astype(np.int64)
    else:
        idx = rows[:, None] * K + np.arange(K)[None, :]
        mask = c.pair_mask[idx] != 0
    drow = (c.dir_map[rows] if c.dir_map is not None else rows) // c.dir_div
    xyz_g = c.xyz[idx].astype(dtype)
    old = O.F32
    O.F32 = dtype                       # w2pers in the working dtype, as aggregate_ref does
    try:
        pers_g = (c.pers[idx].astype(dtype) if c.pers is not None
                  else O.w2pers(xyz_g, c.campos[0].astype(dtype), c.camrot[0].astype(dtype)))
    finally:
        O.F32 = old
    zeros3 = np.zeros(idx.shape + (3,), dtype)
    color_g = zeros3 if c.color is None else c.color[idx].astype(dtype)
    dir_g = zeros3 if c.dir is None else c.dir[idx].astype(dtype)
    conf_g = None if c.conf is None else c.conf[idx].astype(dtype)[..., None]
    Rw = None if c.Rw2c is None else c.Rw2c.astype(dtype)
    params = {k: a.astype(dtype) for k, a in case_params(c).items()}

    def s(a):
        return None if a is None else a[:, None]

    out, rv, w, cc = aggregate(params, s(color_g), Rw, s(dir_g), s(conf_g), s(c.emb[idx].astype(dtype)), s(pers_g),
                               s(xyz_g), s(mask), s(c.sample_p[rows].astype(dtype)), s(c.sample_w[rows].astype(dtype)),
                               s(c.dirs[drow].astype(dtype)), neg_slope=c.neg_slope, act_super=c.act_super,
                               order=c.order, dtype=dtype, mut=mut)
    assert out.dtype == dtype
    feat[:n_eff] = out[:, 0]
    untouched[:n_eff] = ~rv[:, 0]
    return dict(feat=feat, untouched=untouched, rows=rows, weight=np.asarray(w[:, 0], dtype),
                conf=np.asarray(cc[:, 0], dtype))


@functools.lru_cache(maxsize=None)
def ref64_and_noise(base, E, order, masked=False):
    """(float64 reference, e_o32 per block, scale per block): computed once per case and shared."""
    c = case(base, E, order)
    if masked:
        c = masked_case(base, E, order)
    r64, r32 = reference(c, np.float64), reference(c, np.float32)
    assert np.array_equal(r64["untouched"], r32["untouched"])
    wr = ~r64["untouched"]
    b64 = AR._block_views(r64["feat"], r64["weight"], r64["conf"], wr)
    b32 = AR._block_views(r32["feat"], r32["weight"], r32["conf"], wr)
    e = {k: float(np.abs(b32[k].astype(np.float64) - b64[k]).max()) if b64[k].size else 0.0 for k in AR.BLOCKS}
    sc = {k: float(np.abs(b64[k]).max()) if b64[k].size else 0.0 for k in AR.BLOCKS}
    return r64, e, sc


@functools.lru_cache(maxsize=None)
def masked_case(base, E, order):
    c = case(base, E, order)
    m = AR.to_masked(c)
    m.E, m.order = E, order
    return m


def emulate(c, mut=None, dtype=np.float32):
    """What a kernel with the bug ``mut`` leaves in canary-prefilled outputs."""
    r = reference(c, dtype, mut)
    of, ow, oc = AR.canary_outputs(c)
    wr = ~r["untouched"]
    of[:c.n_max][wr] = r["feat"][wr]
    ow[r["rows"]] = r["weight"]
    oc[r["rows"]] = r["conf"]
    return of, ow, oc
