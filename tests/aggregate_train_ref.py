"""TEST INFRASTRUCTURE ONLY -- a torch (CPU) restatement of the training aggregate
on the hand-built sample lists of tests/aggregate_ref.py, with every LeakyReLU
branch pinned from outside, for the training kernels (pnr_aggregate_fwd_train,
_x3, _h2_guarded, _masked) and the whole backward behind train.AggregateFn.

``reference(case, dtype, signs)`` restates the gather the kernels fuse (clamped
rows and the mask, w2pers per pair under the pair's camera, the dirs row and
dir_map, the per-pair Rw2c with slot 0's matrix for the view direction,
used_map) and then writes the MLP out layer by layer: block1.0's point half and
pair half, block1.2, block3.0 with its 7 extras columns, block3.2, the alpha
branch and the K-sum with wt = wn * clamp(conf) (the clamp straight through),
the colour branch.  Every LeakyReLU is ``where(sign, z, slope * z)``.  With
``signs=None`` the sign is the restatement's own ``z > 0``; otherwise the caller
gives the eight boolean tensors (``SIGN_KEYS``) -- in the GPU suite they come from
the kernel's own saved post-activations, which is what the backward reads: it
never recomputes a sign.  Given the signs the backward is an exact linear map of
the upstream gradient, so kernel and reference differ by arithmetic alone; an
fp64 reference with its own signs disagrees with an fp32 kernel on the branch of
every pre-activation within fp32 noise of 0, and one flipped unit moves a weight
gradient by far more than rounding does.  (That the kernel's signs are right is
checked separately: a saved sign may differ from ``z64 > 0`` only where |z64| is
within the measured fp32 noise of that layer.)

It returns feat [n_max, 129], the pre-activations and the gradients of <G, feat>
for a seeded G: per point (emb, colour, dir, conf, with ``xyz_grad`` xyz), the 16
parameters in train._PARAM_NAMES order, per pair (dz1..dz4, dpa, d conf).  Rows
v >= min(n_dev, n_max) and samples without a neighbour contribute nothing.

A point exactly at its sample (|p - s| <= 1e-6, the ``geom`` cases).  The
reference project's forward is 1 / clamp(norm(d), min=1e-6) (point_aggregators.py
:425 under :775-804).  Its autograd gives there: the clamp passes no gradient
below its bound and torch's norm backward is defined as 0 at d = 0, so NO gradient
reaches xyz through the distance weight of that pair (neither its own 1 / norm
nor, through it, the normalising sum), while the PE_5 channels of d = p - s (and
of the perspective deltas) pass their gradient unchanged -- finite, no NaN.  The
restatement below uses the same two torch operations, so its autograd is that
one; k_xyz_bwd's ``nrm > 1e-6f`` branch is the same rule.

``noise(name, signs)`` runs the restatement in float32 and in float64 under the
same signs and returns per tensor e_o32 = max |g32 - g64| and max |g64|: the noise
of fp32 arithmetic on that case, measured on the CPU and never on a kernel.  The
tight bar is aggregate_ref.tight_bar: c * max(e_o32, 2^-22 max|g64|).

``mut`` switches on the emulation of one plausible backward bug (``MUTATIONS``);
tests/test_aggregate_train_ref_host.py shows that each fails a named case on a
named tensor by more than ten times the tight bar.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import aggregate_ref as AR

PARAM_NAMES = ("block1.0.weight", "block1.0.bias", "block1.2.weight", "block1.2.bias",
               "block3.0.weight", "block3.0.bias", "block3.2.weight", "block3.2.bias",
               "alpha_branch.0.weight", "alpha_branch.0.bias",
               "color_branch.0.weight", "color_branch.0.bias", "color_branch.2.weight",
               "color_branch.2.bias", "color_branch.4.weight", "color_branch.4.bias")   # = train._PARAM_NAMES
SIGN_KEYS = ("h1", "h2", "h3", "h4", "hc1", "hc2", "hc3", "pa")   # named after the kernel's saves
POINT_GRADS = ("emb", "color", "dir", "conf", "xyz")
PAIR_GRADS = ("dz1", "dz2", "dz3", "dz4", "dpa", "dconf_pair")
G_SEED = 11

MUTATIONS = ("mask_words_swapped", "empty_dz_kept", "skip_last_tile", "conf_clamp_derivative", "dir_no_rwT",
             "xyz_no_dS", "xyz_cam0", "ignore_used_map", "ignore_n_dev")


def upstream(c, seed=G_SEED):
    """The seeded upstream gradient G [n_max, 129] (float64), one entry per feat entry."""
    return np.random.default_rng(seed + c.n_max).standard_normal((c.n_max, 129))


def mask_neuron(word, bit):
    """pnr_agg_saved.mask: word 2T + h (within a layer's 16), bit r -> the neuron
    32T + 8 (r >> 2) + 4h + (r & 3) (MFMA 32x32 accumulator register r of lane half h)."""
    T, h = word >> 1, word & 1
    return 32 * T + 8 * (bit >> 2) + 4 * h + (bit & 3)


def _swapped_neurons():
    """neuron -> the neuron whose bit a backward reads when it takes word 8h + T for 2T + h."""
    src = np.empty(256, np.int64)
    for w in range(16):
        T, h = w >> 1, w & 1
        for r in range(16):
            src[mask_neuron(w, r)] = mask_neuron(8 * h + T, r)
    return src


class _PinnedLeaky(torch.autograd.Function):
    """where(s_fwd, z, slope z) whose backward multiplies by where(s_bwd, 1, slope):
    the forward's saved bits as the backward reads them (s_bwd is s_fwd unless a
    mutation reads them wrongly)."""

    @staticmethod
    def forward(ctx, z, s_fwd, s_bwd, slope):
        ctx.save_for_backward(s_bwd)
        ctx.slope = slope
        return torch.where(s_fwd, z, z * slope)

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return torch.where(s, g, g * ctx.slope), None, None, None


def _pe(x, freqs, ori=False):
    # networks.py:175-190: bands 2^f, no pi; interleaved sin / cos per (channel, band)
    bands = 2.0 ** torch.arange(freqs, dtype=x.dtype)
    pts = (x[..., None] * bands).reshape(x.shape[:-1] + (-1,))
    if ori:
        return torch.cat([x, torch.sin(pts), torch.cos(pts)], -1)
    return torch.stack([torch.sin(pts), torch.cos(pts)], -1).reshape(pts.shape[:-1] + (pts.shape[-1] * 2,))


def _w2pers(p, campos, camrot):
    """qpiw.py:102-109 per pair: (x / z, y / z, z) of R^T (p - c); campos [..., 3], camrot [..., 3, 3]."""
    xc = ((p - campos)[..., :, None] * camrot).sum(-2)
    return torch.stack([xc[..., 0] / xc[..., 2], xc[..., 1] / xc[..., 2], xc[..., 2]], -1)


def gather_indices(c, mut=None):
    """The index side of the gather (aggregate_ref.reference's): list entry v ->
    sample row, clamped point rows [n, K] and their mask, the dirs row and the camera."""
    n_eff = max(0, min(int(c.n_dev), int(c.n_max)))
    if mut == "ignore_n_dev":
        n_eff = int(c.n_max)
    v = np.arange(n_eff)
    rows = (c.samp_list[v] if c.samp_list is not None else v).astype(np.int64)
    K = c.K
    if c.pidx is not None:
        pid = c.pidx[rows].reshape(n_eff, K)
        mask = pid >= 0
        idx = np.maximum(pid, 0).astype(np.int64)
    else:                                       # pair tables: pair row = row * K + k
        idx = rows[:, None] * K + np.arange(K)[None, :]
        mask = c.pair_mask[idx] != 0
    base = c.dir_map[rows] if c.dir_map is not None else rows
    drow = (base // c.dir_div).astype(np.int64)
    cam = c.ray_cam[drow].astype(np.int64) if c.ray_cam is not None else np.zeros(n_eff, np.int64)
    return SimpleNamespace(n=n_eff, rows=rows, idx=idx, mask=mask, drow=drow, cam=cam)


def reference(case, dtype=np.float64, signs=None, xyz_grad=False, masked=False, mut=None, G=None, params=None):
    """-> dict(feat [n_max,129], untouched [n_max], z: the eight pre-activations (SIGN_KEYS;
    h* [n,K,256], hc* [n,128], pa [n,K]), signs: the branches taken, grads: name -> numpy
    gradient of <G, feat> in ``dtype`` (POINT_GRADS that exist, PARAM_NAMES, PAIR_GRADS [n,K,..]),
    mask [n,K], idx [n,K], n) on a case of aggregate_ref (``masked``: its pair-table twin).
    G: the upstream gradient (default ``upstream(case)``); params: a numpy state dict
    (default the case's)."""
    assert mut is None or mut in MUTATIONS, mut
    c = AR.to_masked(case) if masked else case
    dt = {np.float32: torch.float32, np.float64: torch.float64}[dtype]
    gi = gather_indices(c, mut)
    n, K = gi.n, c.K
    slope = float(c.neg_slope)
    tt = lambda a: torch.from_numpy(np.array(a)).to(dt)   # noqa: E731
    P = {k: tt(v).requires_grad_(True) for k, v in (params if params is not None else AR.params_of(c)).items()
         if k in PARAM_NAMES}
    leaf = {"emb": tt(c.emb).requires_grad_(True)}
    for k in ("color", "dir", "conf"):
        if getattr(c, k) is not None:
            leaf[k] = tt(getattr(c, k)).requires_grad_(True)
    xyz = tt(c.xyz)
    if xyz_grad:
        assert c.pers is None, "pers given is not w2pers(xyz): no xyz gradient on this case"
        leaf["xyz"] = xyz.requires_grad_(True)
    Gn = upstream(c) if G is None else np.asarray(G)
    feat = torch.zeros((c.n_max, 129), dtype=dt)
    untouched = np.ones(c.n_max, bool)
    out = dict(n=n, idx=gi.idx, mask=gi.mask, rows=gi.rows, untouched=untouched)
    if n == 0:
        zero = {k: np.zeros(tuple(t.shape), dtype) for k, t in {**leaf, **P}.items()}
        zero.update({k: np.zeros((0, K, 256), dtype) for k in PAIR_GRADS[:4]})
        zero.update(dpa=np.zeros((0, K), dtype), dconf_pair=np.zeros((0, K), dtype), d_p1=np.zeros((c.N, 256), dtype))
        return dict(out, feat=feat.numpy(), z={}, signs={}, grads=zero)
    idx, mask = torch.from_numpy(gi.idx), torch.from_numpy(gi.mask)
    cam = torch.from_numpy(gi.cam)
    # ---- the gather
    xyz_g = xyz[idx]                                            # [n, K, 3]
    if c.pers is not None:
        pers_g = tt(c.pers)[idx]
    else:
        cp, cr = tt(c.campos), tt(c.camrot)
        pers_g = _w2pers(xyz_g, cp[cam][:, None, :], cr[cam][:, None, :, :])
        if mut == "xyz_cam0":     # the forward's value, the backward through camera 0's w2pers
            p0 = _w2pers(xyz_g, cp[0], cr[0])
            pers_g = pers_g.detach() + (p0 - p0.detach())
    eidx = idx
    if c.used_map is not None and mut == "ignore_used_map":   # d P1 rows taken as point rows: the forward's
        nu = c.used.shape[0] if c.n_used_dev is None else min(c.used.shape[0], c.n_used_dev)   # values, the
        eidx = torch.from_numpy(c.used[gi.idx % nu].astype(np.int64))                          # gradient misplaced
    e = leaf["emb"][idx]
    if eidx is not idx:
        w = leaf["emb"][eidx]
        e = e.detach() + (w - w.detach())
    zeros3 = torch.zeros((n, K, 3), dtype=dt)
    col = leaf["color"][idx] if "color" in leaf else zeros3
    dir_g = leaf["dir"][idx] if "dir" in leaf else zeros3
    sl, slw, rd = tt(c.sample_p[gi.rows]), tt(c.sample_w[gi.rows]), tt(c.dirs[gi.drow])
    if c.rw2c is not None:
        Rpair = tt(c.rw2c).reshape(-1, 3, 3)[idx]              # [n, K, 3, 3]
        Rray = Rpair[:, 0]                                     # slot 0's matrix rotates the view direction
    else:
        Rray = tt(c.Rw2c) if c.Rw2c is not None else torch.eye(3, dtype=dt)
        Rpair = Rray
    rot = lambda x, R: (x[..., None, :] * R).sum(-1)           # noqa: E731  (x @ R^T per row)
    # ---- distances and weights (point_aggregators.py:775-811)
    xd = pers_g[..., 0] * pers_g[..., 2] - (sl[:, 0] * sl[:, 2])[:, None]
    yd = pers_g[..., 1] * pers_g[..., 2] - (sl[:, 1] * sl[:, 2])[:, None]
    zd = pers_g[..., 2] - sl[:, None, 2]
    dw = xyz_g - slw[:, None, :]
    w = mask.to(dt) / torch.clamp(torch.linalg.vector_norm(dw, dim=-1), min=1e-6)
    S = torch.clamp(w.sum(-1, keepdim=True), min=1e-8)
    wn = w / (S.detach() if mut == "xyz_no_dS" else S)
    conf_pair = None
    if "conf" in leaf:
        conf_pair = leaf["conf"].reshape(-1)[idx]
        conf_pair.retain_grad()
        if mut == "conf_clamp_derivative":
            confc = torch.clamp(conf_pair, 1e-4, 1.0)
        else:                                                   # gradiant_clamp (:724-726): identity gradient
            confc = conf_pair - (conf_pair - torch.clamp(conf_pair, 1e-4, 1.0)).detach()
        wt = wn * confc
    else:
        wt = wn
    # ---- the MLP, layer by layer
    sg, z = {}, {}
    swap = torch.from_numpy(_swapped_neurons()) if mut == "mask_words_swapped" else None

    def act(name, pre):
        pre.retain_grad()
        z[name] = pre
        s = pre.detach() > 0
        if signs is not None:
            given = torch.as_tensor(np.asarray(signs[name]))
            if mut == "ignore_n_dev":      # rows past the list take their own signs
                s = torch.cat([given.reshape((-1,) + pre.shape[1:]), s[given.shape[0]:]], 0)
            else:
                s = given.reshape(pre.shape)
        sg[name] = s
        s_bwd = s[..., swap] if (swap is not None and pre.shape[-1] == 256) else s
        return _PinnedLeaky.apply(pre, s, s_bwd, slope)

    W1, W3, C0 = P["block1.0.weight"], P["block3.0.weight"], P["color_branch.0.weight"]
    pe5 = _pe(torch.cat([rot(dw, Rpair), torch.stack([xd, yd, zd], -1)], -1), 5)          # [n, K, 60]
    x1 = torch.cat([e, _pe(e, 3)], -1)                                                       # [n, K, 224]
    h = act("h1", x1 @ W1[:, :224].t() + pe5 @ W1[:, 224:].t() + P["block1.0.bias"])
    h = act("h2", h @ P["block1.2.weight"].t() + P["block1.2.bias"])
    vd = rot(rd, Rray)                                                                      # [n, 3]
    sdir = rot(dir_g, Rpair)
    if mut == "dir_no_rwT":
        sdir.retain_grad()
    ov = vd[:, None, :]
    x3e = torch.cat([col, sdir - ov, (sdir * ov).sum(-1, keepdim=True)], -1)                # [n, K, 7]
    h = act("h3", h @ W3[:, :256].t() + x3e @ W3[:, 256:].t() + P["block3.0.bias"])
    h4 = act("h4", h @ P["block3.2.weight"].t() + P["block3.2.bias"])
    pa = (h4 * P["alpha_branch.0.weight"][0]).sum(-1) + P["alpha_branch.0.bias"][0]        # [n, K]
    pa.retain_grad()
    z["pa"] = pa
    if c.act_super:
        a = torch.nn.functional.softplus(pa - 1)
        sg["pa"] = pa.detach() > 0
    else:
        sg["pa"] = (pa.detach() > 0) if signs is None else torch.as_tensor(np.asarray(signs["pa"])).reshape(pa.shape)
        a = _PinnedLeaky.apply(pa, sg["pa"], sg["pa"], 0.0)
    alpha = (wt * a).sum(-1)
    hid = (wt[..., None] * h4).sum(-2)                                                      # [n, 256]
    if mut == "empty_dz_kept":    # the rows of empty pairs carry a gradient (the value is unchanged)
        hid = hid + ((~mask).to(dt)[..., None] * 0.125 * (h4 - h4.detach())).sum(-2)
    vpe = _pe(vd, 4, ori=True)[:, 3:]                                                        # [n, 24]
    x = act("hc1", hid @ C0[:, :256].t() + vpe @ C0[:, 256:].t() + P["color_branch.0.bias"])
    x = act("hc2", x @ P["color_branch.2.weight"].t() + P["color_branch.2.bias"])
    x = act("hc3", x @ P["color_branch.4.weight"].t() + P["color_branch.4.bias"])
    rv = mask.any(-1)
    rows_f = torch.where(rv[:, None], torch.cat([alpha[:, None], x], -1), torch.zeros((), dtype=dt))
    feat = torch.cat([rows_f, feat[n:]], 0)
    untouched[:n] = ~gi.mask.any(-1)
    # ---- the gradients of <G, feat>
    Gt = torch.from_numpy(Gn).to(dt).clone()
    if mut == "skip_last_tile" and n % AR.TILE_X3:
        Gt[n - n % AR.TILE_X3:n] = 0
    (feat * Gt).sum().backward()
    g = {}
    for k, t in {**leaf, **P}.items():
        g[k] = (torch.zeros_like(t) if t.grad is None else t.grad).numpy()
    if mut == "dir_no_rwT" and "dir" in leaf:
        d = torch.zeros_like(leaf["dir"]).index_put((idx.reshape(-1),), sdir.grad.reshape(-1, 3), accumulate=True)
        g["dir"] = d.numpy()
    for i, k in enumerate(("h1", "h2", "h3", "h4")):
        g[f"dz{i + 1}"] = z[k].grad.numpy()
    g["dpa"] = pa.grad.numpy()
    g["dconf_pair"] = conf_pair.grad.numpy() if conf_pair is not None else np.zeros((n, K), dtype)
    # block1.0's per-point partial d P1[p] = sum of dz1 over the pairs of point p (empty pairs have dz1 = 0)
    g["d_p1"] = torch.zeros((c.N, 256), dtype=dt).index_put((idx.reshape(-1),), z["h1"].grad.reshape(-1, 256),
                                                            accumulate=True).numpy()
    det = lambda t: t.detach().numpy()   # noqa: E731
    out["aux"] = dict(wt=det(wt), wn=det(wn), pe5=det(pe5), x3e=det(x3e), hid=det(hid), vpe=det(vpe))
    return dict(out, feat=feat.detach().numpy(), z={k: t.detach().numpy() for k, t in z.items()},
                signs={k: t.numpy() for k, t in sg.items()}, grads=g)


def noise(case, signs=None, xyz_grad=False, masked=False, G=None):
    """-> (r64, e_o32, scale): the float64 reference under ``signs`` (None: its own; the
    float32 run then takes the float64 run's, so that the two differ by arithmetic
    alone), per gradient tensor and per pre-activation layer (key "z:" + name) e_o32 =
    max |r32 - r64| and scale = max |r64|."""
    r64 = reference(case, np.float64, signs, xyz_grad, masked, G=G)
    if r64["n"] == 0:
        return r64, {k: 0.0 for k in r64["grads"]}, {k: 0.0 for k in r64["grads"]}
    r32 = reference(case, np.float32, r64["signs"] if signs is None else signs, xyz_grad, masked, G=G)
    e, sc = {}, {}
    for k, g64 in r64["grads"].items():
        e[k] = float(np.abs(r32["grads"][k].astype(np.float64) - g64).max()) if g64.size else 0.0
        sc[k] = float(np.abs(g64).max()) if g64.size else 0.0
    for k, z64 in r64["z"].items():
        m = r64["mask"] if z64.ndim >= 2 and z64.shape[:2] == r64["mask"].shape else ~r64["untouched"][:r64["n"]]
        zz, z3 = z64[m], r32["z"][k][m].astype(np.float64)
        e["z:" + k] = float(np.abs(z3 - zz).max()) if zz.size else 0.0
        sc["z:" + k] = float(np.abs(zz).max()) if zz.size else 0.0
    return r64, e, sc


tight_bar = AR.tight_bar
