"""TEST INFRASTRUCTURE ONLY -- hand-built query buffers and a high-precision
restatement for the composite / ray-march kernels of composite.hip.

The kernels give one wave to a ray and two shading slots to each lane (slot
``lane`` and slot ``lane + 64``); the halves are joined by hand-written
hand-overs.  ``make_bufs`` builds seeded, self-consistent query buffers whose
rays put data in both halves (n_filled at 0, 1, 63, 64, 65, SR - 1, SR; valid
slots only at index >= 64, only at slot 0, only at slot SR - 1; more than 8 and
more than 64 valid slots; filled but no valid slot; non-monotone, equal and
widely spaced depths on both sides of the unfilled slots' depth).

``composite_reference`` scatters such buffers into the reference's dense shapes
and applies functions the oracle already pins to the reference's goldens:
``oracle.ray_dist`` (fp32 numpy: the kernel's single fp32 subtraction and its
comparisons on identical values, so the 1e-8 and 2 vsize_z thresholds cannot flip
between the two sides), ``oracle_grad.ray_march_full`` in the requested dtype and
fill_invalid as in ``oracle.render``.  Gradients are torch autograd of the same
function.  ``march_reference`` is the dense ray_march alone.

The cases of tests/test_gpu_composite.py live here so that the CPU test
(tests/test_composite_ref_host.py) can show, for every one of them, that correct
fp32 arithmetic meets the tolerance the GPU test asks of the kernels.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from oracle import oracle as O
from oracle import oracle_grad as OG

F32 = np.float32
VSIZE_Z = 0.004
FEAT_H_PITCH = 136   # PNR_FEAT_H_PITCH (include/pnr.h)

# ------------------------------------------------------------------ tolerance
REL, SCALE = 1e-4, 2e-5   # close(..., rel=1e-4, scale=2e-5) of test_gpu_backward.py
TINY = 1e-30              # absolute term for bg_T / is_bg / d_bg (near fp32's subnormal range)


def err_over_tol(a, ref, abs_=0.0):
    """max over entries of |a - ref| / (SCALE max|ref| + REL |ref| + abs_); a
    non-finite entry of ``a`` gives inf."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0
    a = a.astype(np.float64)
    ref = ref.astype(np.float64)
    if not np.isfinite(a).all():
        return float("inf")
    tol = SCALE * max(float(np.abs(ref).max()), 1e-30) + REL * np.abs(ref) + abs_
    return float((np.abs(a - ref) / tol).max())


class Worst:
    """Worst err / tol per tensor name over the tests of a module."""

    def __init__(self):
        self.w = {}

    def close(self, a, ref, name, abs_=0.0, what=""):
        e = err_over_tol(a, ref, abs_)
        self.w[name] = max(self.w.get(name, 0.0), e)
        print(f"err/tol {what} {name}: {e:.3e}")
        assert e <= 1.0, f"{what} {name}: max err / tol = {e:.3e}"
        return e


# ---------------------------------------------------------------------- cases
DENSE_SR = (1, 2, 63, 64, 65, 127, 128)
DENSE_C = (1, 3, 64, 65, 128, 200)
# (SR, C, bg): each SR and each C with bg and without
DENSE_CASES = ([(sr, c, bg) for sr, c in zip(DENSE_SR, (3, 65, 1, 200, 64, 128, 3)) for bg in (True, False)] +
               [(sr, c, bg) for sr, c, bg in ((128, 1, True), (65, 1, False), (128, 64, True), (127, 64, False),
                                              (65, 65, False), (128, 65, True), (64, 128, True), (128, 128, False),
                                              (128, 200, True), (65, 200, False), (2, 3, False), (63, 3, True))])
DENSE_NR = 40

FUSED_SR = (1, 2, 63, 64, 65, 80, 127, 128)
FUSED_C = (1, 3, 4, 64, 66, 128)
FUSED_R = 48
# (SR, C, bg, unit): each SR with bg and without and with both unit modes, each C likewise
FUSED_CASES = ([(sr, c, bg, unit) for (sr, c), (bg, unit) in
                zip(zip(FUSED_SR, (3, 66, 1, 128, 4, 128, 64, 3)), [(True, 1), (False, 0)] * 4)] +
               [(sr, c, bg, unit) for (sr, c), (bg, unit) in
                zip(zip(FUSED_SR, (4, 1, 64, 3, 128, 66, 1, 66)), [(False, 0), (True, 1)] * 4)] +
               [(128, 128, True, 1), (128, 4, False, 0), (65, 3, True, 0), (127, 128, False, 1), (128, 1, True, 1),
                (65, 64, False, 1), (80, 4, True, 1), (80, 3, False, 0)])
FUSED_HF_CASES = [c for c in FUSED_CASES if c[1] % 2 == 0]
AUX_CASES = ((80, 1), (65, 8), (128, 16))   # (SR, K) of the pnr_march_aux weight cases
WRAPPER_CASE = dict(B=2, R=20, SR=65, C=3, seed=11)
ROW_CAP_CASE = dict(SR=128, K=8, C=3, seed=91)


def case_seed(SR, C):
    """The seed of a (SR, C) case: the CPU and the GPU test build the same inputs."""
    return SR + C


# ------------------------------------------------------------------- dense inputs
def make_dense(NR, SR, C, seed=0, sat=False, fixed=True):
    """Dense ray_march inputs in the goldens' own distribution: sigma uniform in
    (0, 300), dist in (0, 0.01) (sat: up to 0.1, sigma * dist up to 30, opacity
    exactly 1 in fp32), normal features, valid fraction 0.6; plus fixed rays: all
    slots invalid, only slot 0 valid, only slot SR - 1 valid, valid only in the
    upper half (SR > 64)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rf = torch.randn((NR, SR, C + 1), generator=g)
    rf[..., 0] = torch.rand((NR, SR), generator=g) * 300.0
    rd = torch.rand((NR, SR), generator=g) * (0.1 if sat else 0.01)
    rv = (torch.rand((NR, SR), generator=g) < 0.6)
    fixed_rays = {}
    if fixed:
        rv[0] = False
        fixed_rays["all_invalid"] = 0
        if NR > 1:
            rv[1] = False
            rv[1, 0] = True
            fixed_rays["only_slot0"] = 1
        if NR > 2:
            rv[2] = False
            rv[2, SR - 1] = True
            fixed_rays["only_last"] = 2
        if NR > 3 and SR > 64:
            rv[3, :64] = False
            rv[3, 64:] = True
            fixed_rays["upper_only"] = 3
    bg = torch.rand(C, generator=g)
    return dict(rd=rd, rv=rv.to(torch.uint8), rf=rf, bg=bg, fixed=fixed_rays)


def dense_grads(NR, SR, C, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return dict(color=torch.randn((NR, C), generator=g), opacity=torch.randn((NR, SR), generator=g),
                acc_T=torch.randn((NR, SR), generator=g), blend=torch.randn((NR, SR), generator=g),
                bgT=torch.randn((NR,), generator=g))


def march_reference(rd, rv, rf, bg, dtype, grads=None):
    """oracle_grad.ray_march_full in ``dtype``: dict color, opacity, acc_T, blend,
    bgT [NR]; with grads (dict of output gradients, missing = 0): d_feat, d_dist,
    d_bg by autograd of sum_o <out_o, grads_o>."""
    rd_ = rd.to(dtype).clone().requires_grad_(grads is not None)
    rf_ = rf.to(dtype).clone().requires_grad_(grads is not None)
    bg_ = None if bg is None else bg.to(dtype).clone().requires_grad_(grads is not None)
    color, opacity, T, bw, bgT = OG.ray_march_full(rd_, rv.bool(), rf_, bg_)
    out = dict(color=color, opacity=opacity, acc_T=T, blend=bw, bgT=bgT[..., 0])
    if grads is not None:
        loss = sum((out[k] * v.to(dtype)).sum() for k, v in grads.items() if v is not None)
        loss.backward()
        out["d_feat"] = rf_.grad
        out["d_dist"] = rd_.grad
        out["d_bg"] = None if bg_ is None else (bg_.grad if bg_.grad is not None else torch.zeros_like(bg_))
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


# ------------------------------------------------------------------ query buffers
def cameras(n_cams=1):
    """(campos [n,3], camrot [n,3,3]) float32: cameras at different distances, so
    the unfilled slots' depth differs between them."""
    from pointnerf_amd import synthetic as S
    cams = [S.camera(20.0 + 60.0 * i, -30.0, 4.0 - 0.3 * i) for i in range(n_cams)]
    return (np.stack([c[0] for c in cams]).astype(F32), np.stack([c[1] for c in cams]).astype(F32))


def origin_depth(campos, camrot):
    """z of the unfilled slots (sample_loc_w = 0) per camera, [n] float32."""
    return np.array([O.w2pers(np.zeros(3, F32), campos[i], camrot[i])[2] for i in range(campos.shape[0])], F32)


def _forced_rays(SR):
    """(name, n_filled, valid pattern, depth pattern) of the forced rays."""
    specs = []
    for n in sorted({0, 1, 63, 64, 65, SR - 1, SR}):
        if 0 <= n <= SR:
            specs.append((f"n{n}", n, "all" if n == 1 else "rand1", "rand"))
    specs += [("only_slot0", SR, "slot0", "rand"), ("only_last", SR, "last", "rand"),
              ("all_valid", SR, "all", "rand"), ("nine_valid", min(SR, 20), "all", "rand"),
              ("none_valid", min(SR, 10), "none", "rand"), ("nonmono", min(SR, 12), "all", "nonmono"),
              ("equal", min(SR, 12), "all", "equal"), ("gap", min(SR, 12), "all", "gap"),
              ("below", min(SR, 12), "all", "below"), ("above", min(SR, 12), "all", "above"),
              ("straddle", SR, "all", "straddle")]
    if SR > 64:
        specs.append(("upper_only", SR, "upper", "rand"))
        specs.append(("peak", SR, "all", "peak"))
    return specs


def make_bufs(R, SR, K=8, seed=0, n_cams=1, forced=True, n_points=200):
    """Seeded self-consistent query buffers for R rays (torch CPU tensors):
    n_filled [R], ray_off [R+1], vflag [S], valid_off [S+1], ray_vcnt [R], ray_row
    [R+1], sample_p [S,3], sample_w [S,3], pidx [S,K], xyz [n_points,3], campos,
    camrot, ray_cam [R] (None with one camera), names (forced ray -> index)."""
    rng = np.random.default_rng(7000 + 131 * seed + SR)
    campos, camrot = cameras(n_cams)
    zo = origin_depth(campos, camrot)
    ray_cam = rng.integers(0, n_cams, R).astype(np.int32) if n_cams > 1 else np.zeros(R, np.int32)
    specs = _forced_rays(SR) if forced else []
    specs = specs[:R]
    while len(specs) < R:
        specs.append((None, int(rng.integers(0, SR + 1)), "rand", "rand"))
    order = rng.permutation(R)
    specs = [specs[i] for i in order]
    vz = F32(VSIZE_Z)
    n_filled = np.zeros(R, np.int32)
    vfl, zs, names = [], [], {}
    for r, (name, n, vpat, dpat) in enumerate(specs):
        if name:
            names[name] = r
        n_filled[r] = n
        v = np.zeros(n, np.int32)
        if vpat == "all":
            v[:] = 1
        elif vpat in ("rand", "rand1"):
            v[:] = rng.random(n) < 0.6
            if vpat == "rand1" and n and not v.any():
                v[rng.integers(0, n)] = 1
        elif vpat == "slot0":
            v[0] = 1
        elif vpat == "last":
            v[n - 1] = 1
        elif vpat == "upper":
            v[64:] = rng.random(n - 64) < 0.7
            v[n - 1] = 1
        vfl.append(v)
        # depths: steps in units of vsize_z from a start near the unfilled slots' depth
        z0 = zo[ray_cam[r]] + F32(rng.uniform(-1.0, 0.2))
        u = rng.random(n)
        step = rng.uniform(0.25, 1.9, n)
        if dpat == "rand":
            step = np.where(u < 0.1, 0.0, step)                             # equal neighbours
            step = np.where((u >= 0.1) & (u < 0.2), rng.uniform(2.5, 6.0, n), step)   # gaps > 2 vsize_z
            step = np.where((u >= 0.2) & (u < 0.3), -rng.uniform(0.5, 3.0, n), step)  # non-monotone
        elif dpat == "nonmono":
            step = np.where(np.arange(n) % 3 == 1, -2.5, step)
        elif dpat == "equal":
            step = np.where(np.arange(n) % 2 == 1, 0.0, step)
        elif dpat == "gap":
            step = np.where(np.arange(n) % 2 == 1, 4.0, step)
        elif dpat == "below":
            z0 = zo[ray_cam[r]] - F32(0.5)
        elif dpat == "above":
            z0 = zo[ray_cam[r]] + F32(0.1)
        elif dpat == "straddle":
            z0 = zo[ray_cam[r]] - F32(0.4 * n * VSIZE_Z)
        elif dpat == "peak":   # one far sample in the lower half: its depth is the cummax well into the upper half
            step[40] += 60.0
            step[41] -= 60.0
        z = (F32(z0) + np.cumsum(step * VSIZE_Z)).astype(F32)
        zs.append(z)
    vflag = np.concatenate(vfl).astype(np.int32) if R else np.zeros(0, np.int32)
    S = int(vflag.shape[0])
    ray_off = np.concatenate([[0], np.cumsum(n_filled)]).astype(np.int32)
    valid_off = np.concatenate([[0], np.cumsum(vflag)]).astype(np.int32)
    ray_vcnt = np.array([v.sum() for v in vfl], np.int32).reshape(R)
    ray_row = np.concatenate([[0], np.cumsum(ray_vcnt > 0)]).astype(np.int32)
    sample_p = rng.uniform(-0.3, 0.3, (S, 3)).astype(F32)
    if S:
        sample_p[:, 2] = np.concatenate(zs)
    xyz = rng.uniform(-1, 1, (n_points, 3)).astype(F32)
    sample_w = rng.uniform(-1, 1, (S, 3)).astype(F32)
    pidx = rng.integers(0, n_points, (S, K)).astype(np.int32)
    pidx[rng.random((S, K)) < 0.3] = -1
    if S > 2:
        pidx[1] = -1                          # a filled slot without any neighbour
        sample_w[2] = xyz[max(pidx[2, 0], 0)]   # a neighbour at distance 0 (the 1e-6 clamp)
        pidx[2, 0] = max(pidx[2, 0], 0)
    t = torch.from_numpy
    return dict(R=R, SR=SR, K=K, S=S, S_valid=int(valid_off[-1]), R_valid=int(ray_row[-1]),
                n_filled=t(n_filled), ray_off=t(ray_off), vflag=t(vflag), valid_off=t(valid_off),
                ray_vcnt=t(ray_vcnt), ray_row=t(ray_row), sample_p=t(sample_p), sample_w=t(sample_w),
                pidx=t(pidx), xyz=t(xyz), campos=t(campos), camrot=t(camrot),
                ray_cam=t(ray_cam) if n_cams > 1 else None, names=names)


def make_feat(bufs, C, seed=0, bf16=False):
    """Feature rows [S_valid, C+1] in the goldens' distribution: alpha uniform in
    (0, 300), normal channels (bf16: channels rounded to bf16, exact in fp32)."""
    g = torch.Generator().manual_seed(3000 + seed)
    f = torch.randn((bufs["S_valid"], C + 1), generator=g)
    f[:, 0] = torch.rand(bufs["S_valid"], generator=g) * 300.0
    if bf16:
        f[:, 1:] = f[:, 1:].to(torch.bfloat16).float()
    return f


def pack_hf(feat):
    """Rows of FEAT_H_PITCH uint16 (as an int16 tensor) from bf16-exact rows
    [S,C+1]: alpha as one fp32 in halves 0-1, bf16 features in halves 8..8+C-1,
    every other half a bf16 NaN (the kernel must not read them into a result)."""
    S, CF = feat.shape
    rows = np.full((max(S, 1), FEAT_H_PITCH), 0x7FC0, np.uint16)
    rows.view(F32)[:S, 0] = feat[:, 0].numpy()
    bits = feat[:, 1:].to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(feat[:, 1:].to(torch.bfloat16).float().numpy(), feat[:, 1:].numpy()), "not bf16-exact"
    rows[:S, 8:8 + CF - 1] = bits
    return torch.from_numpy(rows.view(np.int16))


def unpack_hf(rows, S, C):
    """The values pnr_composite_fwd_hf reads from pack_hf's rows, [S,C+1] fp32."""
    u = rows.numpy().view(np.uint16)[:S]
    out = np.zeros((S, C + 1), F32)
    out[:, 0] = np.ascontiguousarray(u[:, :2]).view(F32)[:, 0]
    out[:, 1:] = (u[:, 8:8 + C].astype(np.uint32) << 16).view(F32)
    return torch.from_numpy(out)


def scatter_dense(bufs, feat, feat_rows=0):
    """The reference's dense shapes of the buffers: sample_loc [R,SR,3] (z only;
    unfilled slots = oracle.w2pers(0, campos[cam], camrot[cam])[2]), ray_valid
    [R,SR] (rows at or past feat_rows are not valid), (ray, slot, row) of every
    valid sample."""
    R, SR = bufs["R"], bufs["SR"]
    campos, camrot = bufs["campos"].numpy(), bufs["camrot"].numpy()
    zo = origin_depth(campos, camrot)
    cam = bufs["ray_cam"].numpy() if bufs["ray_cam"] is not None else np.zeros(R, np.int64)
    n = bufs["n_filled"].numpy()
    off = bufs["ray_off"].numpy()
    vflag, vo = bufs["vflag"].numpy(), bufs["valid_off"].numpy()
    loc = np.zeros((R, SR, 3), F32)
    rv = np.zeros((R, SR), bool)
    ri, si, rowi = [], [], []
    lim = feat_rows if feat_rows > 0 else np.iinfo(np.int64).max
    zp = bufs["sample_p"].numpy()
    for r in range(R):
        loc[r, :, 2] = zo[cam[r]]
        loc[r, :n[r], 2] = zp[off[r]:off[r] + n[r], 2]
        for s in range(n[r]):
            i = off[r] + s
            if vflag[i] and vo[i] < lim:
                rv[r, s] = True
                ri.append(r)
                si.append(s)
                rowi.append(vo[i])
    idx = tuple(torch.tensor(a, dtype=torch.long) for a in (ri, si, rowi))
    return loc, rv, idx


def composite_reference(bufs, feat, cams, params, dtype, d_color=None):
    """ray_color [R,C], opacity [R,SR], is_bg [R], ray_mask [R] int8, blend [R,SR]
    (and d_feat [S_valid,C+1] for d_color [R,C]; rows no ray reads stay 0) of
    pnr_composite_fwd / _bwd on the buffers.  cams = (campos, camrot) or None for
    the buffers' own; params: dict(vsize_z, unit, bg (tensor or None), feat_rows)."""
    if cams is not None:
        bufs = dict(bufs, campos=torch.as_tensor(cams[0]).reshape(-1, 3), camrot=torch.as_tensor(cams[1]).reshape(-1, 3, 3))
    R, SR = bufs["R"], bufs["SR"]
    CF = feat.shape[1]
    loc, rv, (ri, si, rowi) = scatter_dense(bufs, feat, params.get("feat_rows", 0))
    rdist = O.ray_dist(loc, rv, params["vsize_z"], params["unit"])   # fp32 numpy
    rows = torch.nan_to_num(feat, nan=0.0).to(dtype).clone()   # rows past feat_rows may hold NaN: never gathered
    rows.requires_grad_(d_color is not None)
    dense = torch.zeros((R, SR, CF), dtype=dtype)
    dense = dense.index_put((ri, si), rows[rowi])
    bg = params.get("bg")
    bg_ = None if bg is None else bg.to(dtype)
    rvt = torch.from_numpy(rv)
    color, opacity, T, bw, bgT = OG.ray_march_full(torch.from_numpy(rdist).to(dtype), rvt, dense, bg_)
    mask = bufs["ray_vcnt"] > 0
    out = {"ray_dist": rdist, "ray_valid": rv}
    if d_color is not None:
        (color[mask] * d_color.to(dtype)[mask]).sum().backward()
        out["d_feat"] = rows.grad.detach() if rows.grad is not None else torch.zeros_like(rows)
    # fill_invalid (oracle.render): background colour or 0, opacity 0, is_bg 1, ray_mask 0
    color = color.detach().clone()
    color[~mask] = bg_ if bg_ is not None else 0.0
    opacity = opacity.detach().clone()
    opacity[~mask] = 0.0
    is_bg = bgT.detach()[:, 0].clone()
    is_bg[~mask] = 1.0
    out.update(ray_color=color, opacity=opacity, is_bg=is_bg, ray_mask=mask.to(torch.int8), blend=bw.detach())
    return out


def aux_weight_reference(bufs, dtype=torch.float64):
    """pnr_march_aux's weight [R'',SR,K] in dtype: v_k = 1 / max(|xyz[p_k] -
    sample_w|, 1e-6) for p_k >= 0, else 0, over max(sum v, 1e-8); slots at or past
    n_filled give 0.  Rows in ray_row order."""
    R, SR, K = bufs["R"], bufs["SR"], bufs["K"]
    out = torch.zeros((bufs["R_valid"], SR, K), dtype=dtype)
    xyz, sw, pidx = bufs["xyz"].to(dtype), bufs["sample_w"].to(dtype), bufs["pidx"].long()
    for r in range(R):
        if bufs["ray_vcnt"][r] <= 0:
            continue
        row, n, off = int(bufs["ray_row"][r]), int(bufs["n_filled"][r]), int(bufs["ray_off"][r])
        p = pidx[off:off + n]
        d = torch.linalg.norm(xyz[p.clamp(min=0)] - sw[off:off + n, None, :], dim=-1)
        v = torch.where(p >= 0, 1.0 / d.clamp(min=1e-6), torch.zeros_like(d))
        out[row, :n] = v / v.sum(-1, keepdim=True).clamp(min=1e-8)
    return out


def upper_half_valid(bufs):
    """True when some ray has a valid slot at index >= 64."""
    n, off, vflag = bufs["n_filled"].numpy(), bufs["ray_off"].numpy(), bufs["vflag"].numpy()
    return any(vflag[off[r] + 64:off[r] + n[r]].any() for r in range(bufs["R"]) if n[r] > 64)


# ------------------------------------------------- the two-half algorithm, emulated
# A numpy restatement of the kernels' own algorithm -- two 64-slot halves joined by
# the hand-overs -- with each hand-over removable.  It is not a reference: the CPU
# test uses it to show that the cases separate a kernel with a missing or misplaced
# hand-over from a correct one by more than the tolerance.
HANDOVERS_MARCH = ("tot0", "e1", "bgT", "dP0", "tot1", "last")
HANDOVERS_DIST = ("cm0", "nx0")


def _halves(a):
    return a[:, :64], a[:, 64:]


def two_half_march(rd, rv, rf, bg, grads, drop=None):
    """march_slots / march_slots_bwd and the dense kernels' colour sums in fp64
    numpy on [NR,128] padded slots; drop: the hand-over left out."""
    rd, rf = rd.double().numpy(), rf.double().numpy()
    v = rv.bool().numpy()
    NR, SR = rd.shape
    pad = lambda a: np.concatenate([a, np.zeros((NR, 128 - SR) + a.shape[2:])], 1)   # noqa: E731
    inr = np.arange(128)[None, :] < SR
    sig, dist = pad(rf[..., 0] * v), pad(rd)
    x = np.exp(-sig * dist)
    op = 1 - x
    f = np.where(inr, 1 - op + 1e-10, 1.0)
    f0, f1 = _halves(f)
    i0 = np.cumprod(f0, 1)
    tot0 = i0[:, 63:64] if drop != "tot0" else np.ones((NR, 1))
    i1 = np.cumprod(f1, 1) * tot0
    e0 = np.concatenate([np.ones((NR, 1)), i0[:, :-1]], 1)
    e1 = np.concatenate([tot0 if drop != "e1" else i1[:, :1], i1[:, :-1]], 1)
    P, T = np.concatenate([i0, i1], 1), np.concatenate([e0, e1], 1)
    last = SR - 1
    bgT = P[:, last] if drop != "bgT" else i0[:, min(last, 63)]
    w = op * T
    col = rf[..., 1:]
    color = (w[:, :SR, None] * col).sum(1)
    bgv = None if bg is None else bg.double().numpy()
    if bgv is not None:
        color = color + bgv[None] * bgT[:, None]
    t = torch.from_numpy
    out = dict(color=t(color), opacity=t(op[:, :SR].copy()), acc_T=t(T[:, :SR].copy()), blend=t(w[:, :SR].copy()),
               bgT=t(bgT.copy()))
    if grads is None:
        return out
    g = {k: (grads[k].double().numpy() if grads.get(k) is not None else None) for k in ALL_OUT}
    z = np.zeros((NR, SR))
    dcol = g["color"] if g["color"] is not None else np.zeros(color.shape)
    gw = pad((dcol[:, None, :] * col).sum(-1) + (g["blend"] if g["blend"] is not None else z))
    dox = pad(g["opacity"] if g["opacity"] is not None else z)
    dTx = pad(g["acc_T"] if g["acc_T"] is not None else z)
    dbgT = (g["bgT"] if g["bgT"] is not None else np.zeros(NR)) + (0 if bgv is None else dcol @ bgv)
    dT = gw * op + dTx
    dT0, dT1 = _halves(dT)
    dP0 = np.concatenate([dT0[:, 1:], dT1[:, :1] if drop != "dP0" else np.zeros((NR, 1))], 1)
    dP1 = np.concatenate([dT1[:, 1:], np.zeros((NR, 1))], 1)
    dP = np.concatenate([dP0, dP1], 1)
    s = np.arange(128)[None, :]
    if not (drop == "last" and last >= 64):   # dropped: the `lane + 64 == last` case forgotten
        dP = np.where(s == last, dbgT[:, None], dP)
    dP = np.where(s > last, 0.0, dP)
    q = dP * P
    q0, q1 = _halves(q)
    s1 = np.cumsum(q1[:, ::-1], 1)[:, ::-1]
    tot1 = s1[:, :1] if drop != "tot1" else 0.0
    s0 = np.cumsum(q0[:, ::-1], 1)[:, ::-1] + tot1
    df = np.where(inr, np.concatenate([s0, s1], 1) / f, 0.0)
    do = gw * T - df + dox
    d_feat = np.zeros(rf.shape)
    d_feat[..., 1:] = w[:, :SR, None] * dcol[:, None, :]
    d_feat[..., 0] = (do * x * dist)[:, :SR] * v
    out.update(d_feat=t(d_feat), d_dist=t((do * x * sig)[:, :SR].copy()),
               d_bg=None if bgv is None else t(dcol.T @ bgT))
    return out


ALL_OUT = ("color", "opacity", "acc_T", "blend", "bgT")


def two_half_dist(loc, rv, vsize_z, unit, drop=None):
    """k_composite's ray_dist in fp32 numpy: the cummax as two 64-slot scans with
    the cm0 -> cm1 and nx0 hand-overs (drop: the one left out)."""
    z = np.asarray(loc, F32)[..., 2]
    R, SR = z.shape
    zp = np.concatenate([z, np.full((R, 128 - SR), -np.inf, F32)], 1)
    z0, z1 = _halves(zp)
    cm0 = np.maximum.accumulate(z0, 1)
    cm1 = np.maximum.accumulate(z1, 1)
    if drop != "cm0":
        cm1 = np.maximum(cm1, cm0[:, 63:64])
    nx0 = np.concatenate([cm0[:, 1:], cm1[:, :1] if drop != "nx0" else cm0[:, 63:64]], 1)
    nx1 = np.concatenate([cm1[:, 1:], cm1[:, 63:64]], 1)
    cm, nx = np.concatenate([cm0, cm1], 1)[:, :SR], np.concatenate([nx0, nx1], 1)[:, :SR]
    vz = F32(vsize_z)
    with np.errstate(invalid="ignore"):
        d = np.where(np.arange(SR)[None, :] < SR - 1, (nx - cm).astype(F32), vz)
    m = d < F32(1e-8)
    if unit:
        m = m | (d > F32(2 * vsize_z))
    d = np.where(m, vz, d)
    return np.where(rv, d, F32(0)).astype(F32)


# ------------------------------------------------------------------ device side
class DevBufs:
    """Device copies of make_bufs' tensors and the structs the entry points take."""

    def __init__(self, bufs, dev):
        from pointnerf_amd import _lib as L
        self.L = L
        self.t = {k: v.to(dev).contiguous() for k, v in bufs.items() if torch.is_tensor(v)}
        # never hand the library a null pointer for an empty table
        for k in ("vflag", "sample_p", "sample_w", "pidx"):
            if self.t[k].numel() == 0:
                self.t[k] = torch.zeros((1,) + tuple(self.t[k].shape[1:]), dtype=self.t[k].dtype, device=dev)
        t = self.t
        self.rays = L.Rays()
        self.rays.campos_dev, self.rays.camrot_dev = L.ptr(t["campos"]), L.ptr(t["camrot"])
        self.rays.R = bufs["R"]
        self.rays.ray_cam = L.ptr(t["ray_cam"]) if "ray_cam" in t else None
        self.qp = L.QueryParams()
        self.qp.SR, self.qp.K = bufs["SR"], bufs["K"]
        self.qb = L.QueryBufs()
        for k in ("n_filled", "ray_off", "pidx", "valid_off", "vflag", "ray_vcnt", "ray_row", "sample_w", "sample_p"):
            setattr(self.qb, k, L.ptr(t[k]))

    def cp(self, C, bg, unit, feat_rows=0):
        self._bg = bg
        return self.L.CompositeParams(float(VSIZE_Z), int(unit), int(C), self.L.ptr(bg), int(feat_rows))

    def refs(self):
        return ctypes.byref(self.rays), ctypes.byref(self.qp), ctypes.byref(self.qb)
