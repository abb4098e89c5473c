"""composite.hip's kernels called directly on hand-built buffers, against the
fp64 restatement of tests/composite_ref.py: k_composite (fp32 and bf16 rows),
k_composite_bwd, k_ray_march_dense, k_ray_march_dense_bwd and k_march_aux, at
shading-slot counts on both sides of 64 (one wave per ray, lane l owns slots l
and l + 64) and at every channel-count path.

What the cases are meant to catch:
  * n_filled / SR at 63, 64, 65, 127, 128 and the rays valid only at index >= 64:
    the running product's hand-over (e1 = tot0 on lane 0, tot0 = shfl(i0, 63)),
    the m1 ballot and the sl[u] >= 64 shuffle of k_composite, bgT read from i1;
  * non-monotone / equal / widely spaced depths on both sides of the unfilled
    slots' depth, with 65..128 filled slots: cm1 = max(scan(z1), shfl(cm0, 63))
    and nx0 on lane 63;
  * the backward at SR 64, 65, 128 with gradients in the upper half: dP0[63] =
    dT1[0], tot1 = shfl(s1, 0) and the last = SR - 1 cases of march_slots_bwd;
  * valid only at slot 0 / only at slot SR - 1, more than 8 and more than 64
    valid slots (8 feature rows in flight), filled but none valid, bg NULL, C not
    a multiple of 64 (dense: C > 128), several cameras, feat_rows, the grid-stride
    second pass (more than 16384 rays), R = 0.

Tolerance: |d| <= 2e-5 max|ref| + 1e-4 |ref| per tensor against the fp64
restatement (test_gpu_backward.py's bar for this seam), plus an absolute 1e-30 for
bg_T / is_bg / d_bg; ray_mask and the background rays' outputs are exact.  Every
output has a guard tail that must stay untouched and every call runs twice with
bitwise equal results (no atomics in these kernels).

Worst measured max err / tol per tensor on an MI355X, over all cases (1.0 = the
bar; the fp32 restatement on the CPU, tests/test_composite_ref_host.py, stays
below 3.4e-3 on the same inputs):
  dense march   color 3.7e-3  opacity 2.0e-3  acc_T 1.5e-3  blend 2.0e-3  bgT 1.5e-3
                d_feat 2.0e-3  d_dist 4.3e-3  d_bg 1.1e-2
  wrapper B=2   color 3.5e-3  opacity 1.7e-3  acc_T 1.5e-3  blend 1.3e-3  bgT 3.2e-4
                d_feat 7.7e-4  d_dist 3.0e-3  d_bg 1.4e-3
  fused         ray_color 3.7e-3  opacity 1.9e-3  is_bg 1.5e-3  d_feat 2.2e-3
  march_aux     blend 1.9e-3  weight 1.4e-3
No case needed more than the bar and no kernel bug was found.
"""
import ctypes

import numpy as np
import pytest
import torch

import composite_ref as CR

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -7777.25   # float sentinel (finite: a written value never equals it by chance in these ranges)
SENT_I8 = 85
WORST = CR.Worst()
ABS = {"bgT": CR.TINY, "is_bg": CR.TINY, "d_bg": CR.TINY}
ALL5 = ("color", "opacity", "acc_T", "blend", "bgT")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / tol per tensor (kernels vs fp64):")
    for k, v in sorted(WORST.w.items()):
        print(f"  WORST {k}: {v:.3e}")


def L():
    from pointnerf_amd import _lib
    return _lib


class Out:
    """Outputs with a guard tail of GUARD sentinel elements each."""

    def __init__(self, dev):
        self.dev, self.b = dev, {}

    def new(self, name, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        sent = SENT if dtype == torch.float32 else SENT_I8
        self.b[name] = (torch.full((n + GUARD,), sent, dtype=dtype, device=self.dev), n, tuple(shape), sent)
        return L().ptr(self.b[name][0])

    def __getitem__(self, name):
        full, n, shape, _ = self.b[name]
        return full[:n].view(shape)

    def check_guards(self):
        for name, (full, n, _, sent) in self.b.items():
            assert (full[n:] == sent).all(), f"{name}: guard tail overwritten"

    def untouched(self):
        return all((full == sent).all() for full, _, _, sent in self.b.values())


def twice(fn):
    """Run fn (-> Out) twice: bitwise equal buffers, guard tails intact."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for name in a.b:
        x, y = a.b[name][0], b.b[name][0]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), f"{name}: two runs differ"
    a.check_guards()
    return a


def close(a, ref, name, what):
    # recorded per entry-point family: dense / wrapper / fused / march_aux
    WORST.close(a, ref, f"{what.split()[0]}.{name}", ABS.get(name, 0.0), what)


# ====================================================================== dense march
def _dev(d, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}


def dense_fwd(dd, bg, dev):
    NR, SR = dd["rd"].shape
    C = dd["rf"].shape[-1] - 1

    def run():
        o = Out(dev)
        p = [o.new("color", (NR, C)), o.new("opacity", (NR, SR)), o.new("acc_T", (NR, SR)),
             o.new("blend", (NR, SR)), o.new("bgT", (NR,))]
        L().check(L().lib().pnr_ray_march_fwd(L().ptr(dd["rd"]), L().ptr(dd["rv"]), L().ptr(dd["rf"]), L().ptr(bg),
                                              NR, SR, C, *p, L().stream_ptr(dev)), "pnr_ray_march_fwd")
        return o
    return twice(run)


def dense_bwd(dd, bg, g, keys, want_dist, dev, plain=False):
    """pnr_ray_march_bwd_ex with the output gradients named in keys (others NULL);
    plain: pnr_ray_march_bwd (d_color only)."""
    NR, SR = dd["rd"].shape
    C = dd["rf"].shape[-1] - 1
    gp = [L().ptr(g[k]) if k in keys else None for k in ALL5]

    def run():
        o = Out(dev)
        d_feat = o.new("d_feat", (NR, SR, C + 1))
        d_dist = o.new("d_dist", (NR, SR)) if want_dist else None
        args = (L().ptr(dd["rd"]), L().ptr(dd["rv"]), L().ptr(dd["rf"]), L().ptr(bg), NR, SR, C)
        if plain:
            L().check(L().lib().pnr_ray_march_bwd(*args, gp[0], d_feat, L().stream_ptr(dev)), "pnr_ray_march_bwd")
        else:
            L().check(L().lib().pnr_ray_march_bwd_ex(*args, *gp, d_feat, d_dist, L().stream_ptr(dev)),
                      "pnr_ray_march_bwd_ex")
        return o
    return twice(run)


def colsum(w, x):
    """L.weighted_colsum, in column slices of at most 128 (its limit)."""
    return torch.cat([L().weighted_colsum(w, x[:, c:c + 128].contiguous()) for c in range(0, x.shape[1], 128)])


GRAD_COMBOS = (  # (name, output gradients given, d_ray_dist requested)
    ("color", ("color",), False),
    ("all", ALL5, True),
    ("subset", ("color", "acc_T", "bgT"), True),
    ("all_nodist", ALL5, False),
)


def check_dense(NR, SR, C, bg, dev, sat=False, seed=0, combos=GRAD_COMBOS):
    what = f"dense SR={SR} C={C} bg={bg}" + (" saturated" if sat else "")
    d = CR.make_dense(NR, SR, C, seed=seed, sat=sat)
    g = CR.dense_grads(NR, SR, C, seed=seed)
    bgc = d["bg"] if bg else None
    dd, gd = _dev(d, dev), _dev(g, dev)
    bgd = dd["bg"] if bg else None
    ref = CR.march_reference(d["rd"], d["rv"], d["rf"], bgc, torch.float64)
    if sat:
        assert (ref["opacity"].float() == 1).any()   # opacity exactly 1 in fp32: f = 1e-10
    o = dense_fwd(dd, bgd, dev)
    for k in ALL5:
        assert torch.isfinite(o[k]).all(), f"{what} {k}: not finite"
        close(o[k], ref[k], k, what)
    for name, keys, want_dist in combos:
        grads = {k: g[k] for k in keys}
        r = CR.march_reference(d["rd"], d["rv"], d["rf"], bgc, torch.float64, grads)
        ob = dense_bwd(dd, bgd, gd, keys, want_dist, dev)
        assert torch.isfinite(ob["d_feat"]).all(), f"{what} {name} d_feat: not finite"
        close(ob["d_feat"], r["d_feat"], "d_feat", f"{what} grads={name}")
        if want_dist:
            assert torch.isfinite(ob["d_dist"]).all()
            close(ob["d_dist"], r["d_dist"], "d_dist", f"{what} grads={name}")
        else:
            assert "d_dist" not in ob.b
        if name == "color":
            op = dense_bwd(dd, bgd, gd, keys, False, dev, plain=True)
            assert torch.equal(op["d_feat"].view(torch.int32), ob["d_feat"].view(torch.int32))
        if bg and name in ("color", "all"):
            d_bg = colsum(o["bgT"], gd["color"])
            assert torch.isfinite(d_bg).all()
            close(d_bg, r["d_bg"], "d_bg", f"{what} grads={name}")


@pytest.mark.parametrize("SR,C,bg", CR.DENSE_CASES)
def test_dense_march(cuda, SR, C, bg):
    check_dense(CR.DENSE_NR, SR, C, bg, cuda, seed=CR.case_seed(SR, C))


@pytest.mark.parametrize("SR,C", [(128, 3), (65, 64)])
def test_dense_march_saturated(cuda, SR, C):
    check_dense(CR.DENSE_NR, SR, C, True, cuda, sat=True, seed=CR.case_seed(SR, C))


def test_dense_march_grid_stride(cuda):
    """More rays than the capped grid has waves (4096 blocks x 4): the second pass."""
    check_dense(16384 + 37, 2, 3, True, cuda, seed=5, combos=GRAD_COMBOS[:1])


def test_ray_march_wrapper_two_batches(cuda):
    from pointnerf_amd.ray_march import ray_march
    B, R, SR, C, seed = (CR.WRAPPER_CASE[k] for k in ("B", "R", "SR", "C", "seed"))
    d = CR.make_dense(B * R, SR, C, seed=seed)
    g = CR.dense_grads(B * R, SR, C, seed=seed)
    ref = CR.march_reference(d["rd"], d["rv"], d["rf"], d["bg"], torch.float64, g)
    rd = d["rd"].view(B, R, SR).to(cuda).requires_grad_(True)
    rf = d["rf"].view(B, R, SR, C + 1).to(cuda).requires_grad_(True)
    bg = d["bg"].to(cuda).requires_grad_(True)
    out = ray_march(rd, d["rv"].view(B, R, SR).to(cuda), rf, bg_color=bg)
    color, pcol, opacity, acc_T, blend, bgT, bgbw = out
    assert color.shape == (B, R, C) and blend.shape == (B, R, SR, 1) and bgT.shape == (B, R, 1)
    assert torch.equal(pcol, rf[..., 1:]) and torch.equal(bgbw, bgT)
    got = dict(color=color.reshape(B * R, C), opacity=opacity.reshape(B * R, SR), acc_T=acc_T.reshape(B * R, SR),
               blend=blend.reshape(B * R, SR), bgT=bgT.reshape(B * R))
    for k in ALL5:
        close(got[k], ref[k], k, "wrapper B=2")
    sum((got[k] * g[k].to(cuda)).sum() for k in ALL5).backward()
    close(rf.grad.reshape(B * R, SR, C + 1), ref["d_feat"], "d_feat", "wrapper B=2")
    close(rd.grad.reshape(B * R, SR), ref["d_dist"], "d_dist", "wrapper B=2")
    close(bg.grad, ref["d_bg"], "d_bg", "wrapper B=2")


def test_dense_argument_checks(cuda):
    lib = L().lib()
    NR, C = 4, 3
    d = _dev(CR.make_dense(NR, 128, C, seed=1), cuda)
    g = _dev(CR.dense_grads(NR, 128, C, seed=1), cuda)
    st = L().stream_ptr(cuda)

    def fwd(nr, sr):
        o = Out(cuda)
        p = [o.new("color", (NR, C)), o.new("opacity", (NR, 128)), o.new("acc_T", (NR, 128)),
             o.new("blend", (NR, 128)), o.new("bgT", (NR,))]
        rc = lib.pnr_ray_march_fwd(L().ptr(d["rd"]), L().ptr(d["rv"]), L().ptr(d["rf"]), L().ptr(d["bg"]), nr, sr, C,
                                   *p, st)
        torch.cuda.synchronize()
        return rc, o

    def bwd(nr, sr):
        o = Out(cuda)
        p = [o.new("d_feat", (NR, 128, C + 1)), o.new("d_dist", (NR, 128))]
        rc = lib.pnr_ray_march_bwd_ex(L().ptr(d["rd"]), L().ptr(d["rv"]), L().ptr(d["rf"]), L().ptr(d["bg"]), nr, sr,
                                      C, *[L().ptr(g[k]) for k in ALL5], *p, st)
        torch.cuda.synchronize()
        return rc, o

    for call in (fwd, bwd):
        rc, o = call(0, 128)       # NR = 0: OK, nothing written
        assert rc == L().PNR_OK and o.untouched()
        for sr in (0, 129):        # refused
            rc, o = call(NR, sr)
            assert rc == L().PNR_EINVAL and o.untouched()


# ================================================================= fused composite
def fused_fwd(db, cp, feat_d, dev, hf=False):
    R, SR, C = db.rays.R, db.qp.SR, cp.C

    def run():
        o = Out(dev)
        p = [o.new("ray_color", (R, C)), o.new("opacity", (R, SR)), o.new("is_bg", (R,)),
             o.new("ray_mask", (R,), torch.int8)]
        fn = L().lib().pnr_composite_fwd_hf if hf else L().lib().pnr_composite_fwd
        L().check(fn(*db.refs(), ctypes.byref(cp), L().ptr(feat_d), *p, L().stream_ptr(dev)), "pnr_composite_fwd")
        return o
    return twice(run)


def fused_bwd(db, cp, feat_d, d_color_d, rows, dev):
    def run():
        o = Out(dev)
        d_feat = o.new("d_feat", (rows, cp.C + 1))
        L().check(L().lib().pnr_composite_bwd(*db.refs(), ctypes.byref(cp), L().ptr(feat_d), L().ptr(d_color_d),
                                              d_feat, L().stream_ptr(dev)), "pnr_composite_bwd")
        return o
    return twice(run)


def aux(db, dev, rows, xyz=None, opacity=None, rows_max=None, weight=True, blend=True):
    SR, K = db.qp.SR, db.qp.K

    def run():
        o = Out(dev)
        w = o.new("weight", (rows, SR, K)) if weight else None
        b = o.new("blend", (rows, SR)) if blend else None
        L().check(L().lib().pnr_march_aux(*db.refs(), L().ptr(xyz), L().ptr(opacity),
                                          rows if rows_max is None else rows_max, w, b, L().stream_ptr(dev)),
                  "pnr_march_aux")
        return o
    return twice(run)


def check_fwd_out(o, ref, b, what):
    mask = b["ray_vcnt"] > 0
    assert torch.equal(o["ray_mask"].cpu(), ref["ray_mask"]), f"{what}: ray_mask"
    for k in ("ray_color", "opacity", "is_bg"):
        got = o[k].cpu()
        assert torch.isfinite(got).all(), f"{what} {k}: not finite"
        # background rays: exact (colour = bg or 0, opacity 0, is_bg 1)
        assert torch.equal(got[~mask], ref[k][~mask].float()), f"{what} {k}: background rays"
        close(got, ref[k], k, what)


def check_fused(b, C, bg, unit, dev, seed=0, feat_rows=0, hf=None, bwd=True, aux_blend=True):
    SR, R = b["SR"], b["R"]
    what = f"fused SR={SR} C={C} bg={bg} unit={unit}"
    hf = (C % 2 == 0) if hf is None else hf
    feat = CR.make_feat(b, C, seed=seed, bf16=hf)
    g = torch.Generator().manual_seed(4000 + seed)
    d_color = torch.randn((R, C), generator=g)
    bgc = torch.rand(C, generator=g) if bg else None
    params = dict(vsize_z=CR.VSIZE_Z, unit=unit, bg=bgc, feat_rows=feat_rows)
    ref = CR.composite_reference(b, feat, None, params, torch.float64, d_color)
    db = CR.DevBufs(b, dev)
    cp = db.cp(C, bgc.to(dev) if bg else None, unit, feat_rows)
    Sv = b["S_valid"]
    lim = feat_rows if feat_rows > 0 else Sv
    feat_in = feat.clone()
    feat_in[lim:] = float("nan")     # rows at or past feat_rows must not reach a result
    feat_d = feat_in.to(dev) if Sv else torch.zeros((1, C + 1), device=dev)
    o = fused_fwd(db, cp, feat_d, dev)
    check_fwd_out(o, ref, b, what)
    if hf:
        rows_h = CR.pack_hf(feat)
        rows_h[lim:] = 0x7FC0        # bf16 NaN everywhere, alpha included
        oh = fused_fwd(db, cp, rows_h.to(dev), dev, hf=True)
        check_fwd_out(oh, ref, b, what + " hf")
    if bwd:
        rows = max(Sv, 1)
        ob = fused_bwd(db, cp, feat_d, d_color.to(dev), rows, dev)
        got = ob["d_feat"].cpu()
        assert (got[:lim] != SENT).all(), f"{what}: d_feat rows left unwritten"
        assert (got[lim:] == SENT).all(), f"{what}: d_feat rows at or past feat_rows written"
        assert torch.isfinite(got[:lim]).all()
        close(got[:lim], ref["d_feat"][:lim], "d_feat", what)
    if aux_blend and b["R_valid"]:
        mask = b["ray_vcnt"] > 0
        oa = aux(db, dev, b["R_valid"], opacity=o["opacity"].contiguous(), weight=False)
        close(oa["blend"].cpu(), ref["blend"][mask], "blend", what + " march_aux")
    return o, ref, db


@pytest.mark.parametrize("SR,C,bg,unit", CR.FUSED_CASES)
def test_fused_composite(cuda, SR, C, bg, unit):
    b = CR.make_bufs(CR.FUSED_R, SR, seed=CR.case_seed(SR, C))
    assert SR <= 64 or CR.upper_half_valid(b)
    check_fused(b, C, bg, unit, cuda, seed=CR.case_seed(SR, C))


def test_fused_composite_three_cameras(cuda):
    b = CR.make_bufs(CR.FUSED_R, 128, seed=77, n_cams=3)
    assert b["ray_cam"] is not None and len(set(b["ray_cam"].tolist())) == 3
    check_fused(b, 66, True, 1, cuda, seed=77)
    check_fused(b, 66, False, 0, cuda, seed=77)
    # and the per-ray depth matters (unit 0: the last sample below it gets the whole
    # distance to it): with every ray on camera 0 the result differs
    one = dict(b, ray_cam=torch.zeros_like(b["ray_cam"]))
    feat = CR.make_feat(b, 66, seed=77, bf16=True)
    p = dict(vsize_z=CR.VSIZE_Z, unit=0, bg=None, feat_rows=0)
    assert not torch.equal(CR.composite_reference(b, feat, None, p, torch.float64)["opacity"],
                           CR.composite_reference(one, feat, None, p, torch.float64)["opacity"])


def test_fused_composite_feat_rows(cuda):
    """feat_rows = S_valid - 7 on full-sized buffers: the last 7 valid samples
    count as not valid, their (NaN) rows are not read and their d_feat rows keep
    the sentinel."""
    b = CR.make_bufs(CR.FUSED_R, 80, seed=78)
    check_fused(b, 128, True, 1, cuda, seed=78, feat_rows=b["S_valid"] - 7)


def test_fused_composite_grid_stride(cuda):
    b = CR.make_bufs(16384 + 37, 2, seed=79, forced=False)
    check_fused(b, 3, True, 1, cuda, seed=79, hf=False)


def test_fused_composite_empty_batch(cuda):
    b = CR.make_bufs(0, 80, seed=1)
    db = CR.DevBufs(b, cuda)
    bg = torch.rand(4, device=cuda)
    cp = db.cp(4, bg, 1)
    feat = torch.zeros((1, 5), device=cuda)
    o = Out(cuda)
    p = [o.new("ray_color", (1, 4)), o.new("opacity", (1, 80)), o.new("is_bg", (1,)), o.new("ray_mask", (1,), torch.int8)]
    st = L().stream_ptr(cuda)
    assert L().lib().pnr_composite_fwd(*db.refs(), ctypes.byref(cp), L().ptr(feat), *p, st) == L().PNR_OK
    rows_h = torch.zeros((1, CR.FEAT_H_PITCH), dtype=torch.int16, device=cuda)
    assert L().lib().pnr_composite_fwd_hf(*db.refs(), ctypes.byref(cp), L().ptr(rows_h), *p, st) == L().PNR_OK
    d_feat = o.new("d_feat", (1, 5))
    assert L().lib().pnr_composite_bwd(*db.refs(), ctypes.byref(cp), L().ptr(feat), L().ptr(bg), d_feat,
                                       st) == L().PNR_OK
    w = o.new("weight", (1, 80, 8))
    assert L().lib().pnr_march_aux(*db.refs(), L().ptr(feat), None, 1, w, None, st) == L().PNR_OK
    torch.cuda.synchronize()
    assert o.untouched()


@pytest.mark.parametrize("SR,K", CR.AUX_CASES)
def test_march_aux_weight(cuda, SR, K):
    b = CR.make_bufs(CR.FUSED_R, SR, K=K, seed=SR + K)
    db = CR.DevBufs(b, cuda)
    ref = CR.aux_weight_reference(b)
    o = aux(db, cuda, b["R_valid"], xyz=db.t["xyz"], blend=False)
    got = o["weight"].cpu()
    assert torch.isfinite(got).all() and (got != SENT).all()
    close(got, ref, "weight", f"march_aux SR={SR} K={K}")
    assert (got[ref == 0] == 0).all()   # empty neighbours and slots at or past n_filled: exactly 0


def test_march_aux_row_cap_and_null_outputs(cuda):
    SR, K, C, seed = (CR.ROW_CAP_CASE[k] for k in ("SR", "K", "C", "seed"))
    b = CR.make_bufs(CR.FUSED_R, SR, K=K, seed=seed)
    o, ref, db = check_fused(b, C, True, 1, cuda, seed=seed, bwd=False, aux_blend=False)
    Rv = b["R_valid"]
    mask = b["ray_vcnt"] > 0
    op = o["opacity"].contiguous()
    wref, bref = CR.aux_weight_reference(b), ref["blend"][mask]
    both = aux(db, cuda, Rv, xyz=db.t["xyz"], opacity=op)
    close(both["weight"].cpu(), wref, "weight", "march_aux both")
    close(both["blend"].cpu(), bref, "blend", "march_aux both")
    # each output may be NULL separately (and then its input too)
    only_w = aux(db, cuda, Rv, xyz=db.t["xyz"], blend=False)
    only_b = aux(db, cuda, Rv, opacity=op, weight=False)
    assert torch.equal(only_w["weight"], both["weight"]) and torch.equal(only_b["blend"], both["blend"])
    assert L().lib().pnr_march_aux(*db.refs(), L().ptr(db.t["xyz"]), L().ptr(op), Rv, None, None,
                                   L().stream_ptr(cuda)) == L().PNR_OK
    # rows_max = R'' - 3: rows past it keep the sentinel (buffers are full-sized)
    cap = aux(db, cuda, Rv, xyz=db.t["xyz"], opacity=op, rows_max=Rv - 3)
    for k, r in (("weight", wref), ("blend", bref)):
        got = cap[k].cpu()
        assert (got[Rv - 3:] == SENT).all() and (got[:Rv - 3] != SENT).all()
        assert torch.equal(got[:Rv - 3], both[k].cpu()[:Rv - 3])
