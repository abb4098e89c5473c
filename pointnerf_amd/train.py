"""Autograd through the HIP path (the per-scene finetune step;
DESIGN.md section 26 describes this host layer).

``AggregateFn`` and ``CompositeFn`` are torch.autograd.Functions.  AggregateFn's
forward runs one of the training aggregates (``_FORWARD``): the per-pair chain on
f16-split MFMA (``pnr_aggregate_fwd_train_h2_guarded``, train_precision fp32h2:
the default), on bf16-split MFMA (``pnr_aggregate_fwd_train_x3``, fp32x3) or on
native-fp32 MFMA (``pnr_aggregate_fwd_train``, fp32; ``_masked`` for the
PointAggregator.forward seam).  CompositeFn's runs ``pnr_composite_fwd``.

The backward through the aggregator comes in two forms that issue the same
kernels in the same order:

  * one native call, ``pnr_aggregate_bwd_step_h2`` (csrc/train_step.hip): fp32h2
    with a used-point list and no xyz gradient -- the product path;
  * the Python sequence below, for every other case, and the native call's
    reference (tests/test_gpu_backward.py).  ``AggregateFn.backward`` is a plan
    (``_BwdPlan``) and these stages (``_Backward``):

  colour_branch        pnr_color_dz, then per layer the weight gradient dW = dZ^T X
                       (pnr_gemm_tn_x3 / _h2, bias = column sums) and dX = dZ W with
                       the LeakyReLU derivative fused (pnr_gemm_nn / _h2); d hid
  pairs_chain          pnr_aggregate_bwd_pairs(_x3 | _h2): the fused per-pair dX
                       chain on MFMA -- alpha branch + K-sum backward, block3.2^T /
                       block3.0^T / block1.2^T, LeakyReLU masks, per-pair weight /
                       conf terms
  points_from_pairs    pnr_group_pairs, then the per-point sums in pair order (no
                       float atomics, on every chain): d conf, block1.0's per-point
                       partial d P1 and the block3.0 extras' d colour / d dir
  pair_weight_grads    dW = dZ^T X over all pairs: block3.2, block3.0 (+ its extras
                       columns), block1.2, the alpha branch
  block1_point_half    dW1[:, :224] = dP1^T X1, dW1[:, 224:] = dz1^T PE_5,
                       d emb = PE_3 backward of dP1 W1[:, :224]
  xyz                  d PE_5 = dz1 W1[:, 224:], then pnr_aggregate_bwd_xyz

matching the autograd of point_aggregators.py:729-816 / 488-646,
gradiant_clamp (:724-726), the gather (neural_points.py:788-799) and
ray_march (diff_ray_marching.py:509-555).  Gradients are produced for
points_embeding, points_color, points_dir, points_conf and every aggregator
parameter; xyz gradients (xyz_grad) through pnr_aggregate_bwd_xyz.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, NamedTuple

import torch

from . import _lib as L
from .aggregator import frag_pack, frag_pack_x3
from .querier import COUNT_N_USED, COUNT_S_VALID

# fp32h2 training: the backward's three dX GEMMs (k_pairs_bwd) on split-f16 MFMA
# as well (False: on fp32x3, the round-5 product) -- DESIGN.md section 10.
BWD_H2 = True
# fp32h2 training with a used-point list (the renderer's training forward): the
# whole backward through the aggregator as one native call
# (pnr_aggregate_bwd_step_h2) instead of the Python sequence below -- the same
# kernels, ~60 fewer host-side calls per step.
NATIVE_BWD = True

TRAIN_PRECISIONS = ("fp32", "fp32x3", "fp32h2")

_PARAM_NAMES = ("block1.0.weight", "block1.0.bias", "block1.2.weight", "block1.2.bias",
                "block3.0.weight", "block3.0.bias", "block3.2.weight", "block3.2.bias",
                "alpha_branch.0.weight", "alpha_branch.0.bias",
                "color_branch.0.weight", "color_branch.0.bias", "color_branch.2.weight",
                "color_branch.2.bias", "color_branch.4.weight", "color_branch.4.bias")


def agg_params(agg) -> list:
    d = dict(agg.named_parameters())
    return [d[n] for n in _PARAM_NAMES]


BWD_H2_PAD = 3   # k_pairs_bwd<2> loads 3 k-steps ahead (kX3D)


class BwdPacks(NamedTuple):
    """The weights of one pnr_aggregate_bwd_pairs(_x3 | _h2) call."""
    mlp: L.MlpBwd         # fp32 chain: its transposed fragment packs; w3e as packed_bwd was asked
    split: Any            # x3: L.MlpBwdX3 (frag_pack_x3); h2: L.MlpBwdH2 (pnr_pack_bwd_h2); fp32: None
    w3e: torch.Tensor     # block3.0's extras columns W3[:, 256:263], row-major (pnr_aggregate_bwd_extras_rows)
    keep: dict            # the tensors the structs point into


def packed_bwd(agg, chain: str, pairs_w3e: bool) -> BwdPacks:
    """Transposed fragment packs for the dX chain ("fp32" | "x3" | "h2"): native-fp32
    packs, split-bf16 packs, or the split-f16 packs of pnr_pack_bwd_h2 (one launch,
    shifts picked on the device).  pairs_w3e: the pairs pass gets w3e (given d colour /
    d dir buffers it then makes the block3.0 extras' gradients itself, by float
    atomics); else its w3e is NULL."""
    with torch.no_grad():
        W3 = agg.block3[0].weight
        t = dict(w3e=W3[:, 256:263].float().contiguous())
        w3e = t["w3e"].data_ptr() if pairs_w3e else None
        if chain == "h2":
            dev = W3.device
            w4, w2 = agg.block3[2].weight.float().contiguous(), agg.block1[2].weight.float().contiguous()
            w3 = W3.float()
            if w3.stride(1) != 1:
                w3 = w3.contiguous()
            per = (16 + BWD_H2_PAD) * 2048
            t["packs"] = torch.empty(3 * per * 2, dtype=torch.int32, device=dev)   # 3 x per x 8 B
            t["scale"] = torch.empty(4, dtype=torch.float32, device=dev)
            L.check(L.lib().pnr_pack_bwd_h2(L.ptr(w4), L.ptr(w3), w3.stride(0), L.ptr(w2), BWD_H2_PAD,
                                            L.ptr(t["scale"]), L.ptr(t["packs"]), t["packs"].numel() * 4,
                                            L.stream_ptr(dev)), "pnr_pack_bwd_h2")
            t.update(w4=w4, w3=w3, w2=w2)
            base = t["packs"].data_ptr()
            split = L.MlpBwdH2(base, base + per * 8, base + 2 * per * 8, t["scale"].data_ptr())
            return BwdPacks(L.MlpBwd(None, None, None, w3e), split, t["w3e"], t)
        mats = dict(w4t=agg.block3[2].weight.t(), w3t=W3[:, :256].t(), w2t=agg.block1[2].weight.t())
        if chain == "x3":
            t.update({k + "x": frag_pack_x3(v) for k, v in mats.items()})
        else:
            t.update({k: frag_pack(v) for k, v in mats.items()})
    if chain == "x3":
        split = L.MlpBwdX3(*(t[k].data_ptr() for k in ("w4tx", "w3tx", "w2tx")))
        return BwdPacks(L.MlpBwd(None, None, None, w3e), split, t["w3e"], t)
    return BwdPacks(L.MlpBwd(*(t[k].data_ptr() for k in ("w4t", "w3t", "w2t")), w3e), None, t["w3e"], t)


class Saved:
    """Device activations kept by pnr_aggregate_fwd_train (pnr_agg_saved)."""

    def __init__(self, n_max: int, device, n_dev=None, n_x1: int = 0):
        n = max(int(n_max), 1)
        f = dict(dtype=torch.float32, device=device)
        P = n * 8
        self.t = dict(h1=torch.empty((P, 256), **f), h2=torch.empty((P, 256), **f),
                      h3=torch.empty((P, 256), **f), h4=torch.empty((P, 256), **f),
                      pe5=torch.empty((P, 64), **f), x3e=torch.empty((P, 32), **f), pa=torch.empty(P, **f),
                      wt=torch.empty(P, **f), wn=torch.empty(P, **f),
                      prow=torch.empty(P, dtype=torch.int32, device=device),
                      hid=_rows_zeroed((n, 256), n_dev, device), vpe=torch.empty((n, 24), **f),
                      hc1=torch.empty((n, 128), **f), hc2=torch.empty((n, 128), **f),
                      hc3=torch.empty((n, 128), **f), vmask=torch.empty(n, dtype=torch.int32, device=device),
                      mask=torch.empty((P, 64), dtype=torch.int16, device=device),
                      dz_absmax=torch.zeros(6, dtype=torch.int32, device=device),   # |dz1..dz4|, |dpa|, |d_p1|
                      # [emb, PE_3(emb)] of the used points (fp32h2 forward's k_point_pre_h2; ABI 23)
                      x1=torch.empty((int(n_x1), 224), **f) if n_x1 else None)
        self.c = L.AggSaved(*(L.ptr(self.t[k]) for k, _ in L.AggSaved._fields_))

    def absmax(self, i: int):
        """[1] int32 view: float bits of max |dz_{i+1}| (i < 4), |dpa| (4), |d_p1| (5)."""
        return self.t["dz_absmax"][i:i + 1]

    def __getitem__(self, k):
        return self.t[k]


def _rows_zeroed(shape, n_dev, device):
    """fp32 [rows, cols] whose first *n_dev rows are zero (pnr_zero_rows: the
    device-counted part of a capacity-sized buffer, no host read), or all rows
    zero when n_dev is None / 0.  Rows past the count are never read."""
    if not n_dev:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    t = torch.empty(shape, dtype=torch.float32, device=device)
    L.check(L.lib().pnr_zero_rows(L.ptr(t), t.shape[1] * 4, L.c_void_p(n_dev), t.shape[0], L.stream_ptr(device)),
            "pnr_zero_rows")
    return t


def used_points_buffers(n_points: int, device):
    """(flags, used_map, used, scratch) of pnr_used_points for a table of n_points rows."""
    i32 = dict(dtype=torch.int32, device=device)
    flags, used_map, used = (torch.empty(n_points, **i32) for _ in range(3))
    return flags, used_map, used, L.scratch("pnr_used_points_scratch_bytes", n_points, device=device)


def used_points_device(bufs, K: int, n_points: int, kept=None):
    """pnr_used_points on a query's buffers, count into bufs.counts[COUNT_N_USED] (read with the other
    counts by the caller's one read_counts()): (used [N] buffer, used_map [N]) -- slice used[:n_used]
    after the read.  kept: the caller's used_points_buffers(n_points), reused from call to call."""
    dev = bufs.pidx.device
    flags, used_map, used, scratch = kept or used_points_buffers(n_points, dev)
    cap = bufs.pidx.numel() // K
    L.check(L.lib().pnr_used_points(L.ptr(bufs.pidx), L.ptr(bufs.counts), K, cap, n_points, L.ptr(flags),
                                    L.ptr(used_map), L.ptr(used), L.c_void_p(bufs.count_ptr(COUNT_N_USED)),
                                    L.ptr(scratch), scratch.numel(), L.stream_ptr(dev)), "pnr_used_points")
    return used, used_map


def used_points(pidx: torch.Tensor, n_points: int):
    """(used, used_map): sorted point rows referenced by a query's sample_pidx
    and the inverse map (-1 = unreferenced) -- pnr_points.used / used_map."""
    ids = pidx[pidx >= 0]
    used = torch.unique(ids).to(torch.int32)
    used_map = torch.full((n_points,), -1, dtype=torch.int32, device=pidx.device)
    used_map[used.long()] = torch.arange(used.numel(), dtype=torch.int32, device=pidx.device)
    return used, used_map


class UsedPoints(NamedTuple):
    """The point rows one batch references (pnr_used_points)."""
    rows: torch.Tensor        # int32 [capacity]: the referenced rows, ascending; the first count_dev[0] are valid
    row_map: torch.Tensor     # int32 [N]: row -> its position in rows, -1 = unreferenced
    count_dev: torch.Tensor   # int32 [1] on the device: how many


class PointTables(NamedTuple):
    """The point tables an aggregate reads without differentiating them (fp32, contiguous)."""
    xyz: torch.Tensor
    pers: Any = None      # [N,3] perspective coordinates (the seam's gathered pairs; else made from campos / camrot)
    campos: Any = None
    camrot: Any = None
    rw2c: Any = None      # per-point Rw2c [N,9], or None for the aggregator's uniform matrix


@dataclass(eq=False)
class AggSpec:
    """Non-tensor description of one aggregate call (structs + keep-alive)."""
    agg: Any                       # the PointAggregator
    samples: L.Samples
    n: int                         # sample rows (with counts: their capacity)
    points: PointTables
    pair_mask: Any = None          # uint8 [n * K]: the seam's sample_pnt_mask (fp32 only)
    used: UsedPoints | None = None
    precision: str = "fp32"        # the forward's per-pair chain: one of TRAIN_PRECISIONS
    counts: Any = None             # querier.CountsHandle: n / used are then capacities, the true counts
                                   # on the device (read by the backward, never the forward)
    keep: tuple = ()
    keep_saved: bool = False       # tests: leave the forward's activations in saved
    # written by AggregateFn.forward:
    saved: Saved | None = None     # with keep_saved, the kept activations of the forward
    h2_fallback: bool = False      # fp32h2: an earlier forward's range flag was found raised (that call
                                   # ran its native-fp32 fallback on the device)

    def __post_init__(self):
        self.n = int(self.n)
        if self.precision not in TRAIN_PRECISIONS:
            raise L.PnrError(f"AggSpec: precision {self.precision!r}: one of {TRAIN_PRECISIONS}")
        if self.pair_mask is not None and self.precision != "fp32":
            raise L.PnrError(f"AggSpec: a pair mask runs the fp32 forward only, not {self.precision!r}")


# forward -> (its entry point, also the name L.check reports; the aggregator's extra split pack)
_FORWARD = {
    "masked": ("pnr_aggregate_fwd_train_masked", None),
    "fp32": ("pnr_aggregate_fwd_train", None),
    "fp32x3": ("pnr_aggregate_fwd_train_x3", "packed_x3"),
    "fp32h2": ("pnr_aggregate_fwd_train_h2_guarded", "packed_h2_train"),
}


class AggregateFn(torch.autograd.Function):
    """feat[n_max, 129] = aggregate(point tables, MLP); differentiable in emb,
    color, dir, conf, the 16 aggregator parameters and -- when xyz is given
    (--xyz_grad 1; the fused renderer path) -- the point positions."""

    @staticmethod
    def forward(ctx, spec: AggSpec, emb, color, dirs, conf, xyz, *params):
        dev = emb.device
        agg = spec.agg
        s = spec.samples
        n_max = int(s.n_max)
        N = emb.shape[0]
        tabs = [emb.detach().contiguous(), None if color is None else color.detach().contiguous(),
                None if dirs is None else dirs.detach().contiguous(),
                None if conf is None else conf.detach().reshape(-1).contiguous()]
        pt = spec.points
        pts = L.Points(N, pt.xyz.data_ptr(), L.ptr(pt.pers), tabs[0].data_ptr(), L.ptr(tabs[1]),
                       L.ptr(tabs[2]), L.ptr(tabs[3]), L.ptr(pt.campos), L.ptr(pt.camrot))
        pts.rw2c = L.ptr(pt.rw2c)
        n_p1 = N
        if spec.used is not None:   # rows.numel() is the capacity, the count is on the device
            u = spec.used
            pts.used, pts.n_used, pts.used_map = u.rows.data_ptr(), u.rows.numel(), u.row_map.data_ptr()
            pts.n_used_dev = u.count_dev.data_ptr()
            n_p1 = u.rows.numel()
        which = "masked" if spec.pair_mask is not None else spec.precision
        entry, extra_pack = _FORWARD[which]
        run_h2 = which == "fp32h2"
        if run_h2:
            # an earlier step's raised flag (its fallback already ran): shifts re-picked now
            spec.h2_fallback = agg.h2_train_poll()
        # every pack of the step in one launch (the optimizer changed the weights)
        agg.packed_train(h2=run_h2)
        mlp, keepw = agg.packed()
        # fp32h2 with a used-point list: the forward also keeps block1.0's point-half inputs
        sv = Saved(n_max, dev, n_dev=s.n_dev, n_x1=n_p1 if (run_h2 and spec.used is not None) else 0)
        feat = _rows_zeroed((max(n_max, 1), 129), s.n_dev, dev)
        scratch = L.aggregate_scratch(max(n_max, 1), max(n_p1, 1), dev)
        extra, keepx = getattr(agg, extra_pack)() if extra_pack else (None, None)
        # after the fp32 packs: the pair mask, or the split packs
        mid = (L.ptr(spec.pair_mask),) if which == "masked" else () if extra is None else (ctypes.byref(extra),)
        L.check(getattr(L.lib(), entry)(ctypes.byref(pts), ctypes.byref(s), ctypes.byref(mlp), *mid,
                                        ctypes.byref(sv.c), L.ptr(feat), None, None, L.ptr(scratch),
                                        scratch.numel() * 4, L.stream_ptr(dev)), entry)
        if run_h2:
            agg.h2_train_launched()
        ctx.spec, ctx.sv, ctx.pts, ctx.tabs, ctx.mlp, ctx.keepw = spec, sv, pts, tabs, mlp, (keepw, keepx)
        if spec.keep_saved:
            spec.saved = sv
        ctx.has = (color is not None, dirs is not None, conf is not None)
        ctx.xyz_shape = None if xyz is None else xyz.shape
        ctx.shapes = (emb.shape, None if conf is None else conf.shape)
        ctx.save_for_backward(*params)
        return feat

    @staticmethod
    def backward(ctx, d_feat):
        plan = _BwdPlan.of(ctx)
        d_feat = d_feat.contiguous()
        if plan.native:
            return _native_bwd_h2(ctx, ctx.spec, d_feat, plan.n, plan.n_used, ctx.saved_tensors)
        b = _Backward(ctx, d_feat, plan)
        b.colour_branch()
        b.pairs_chain()
        b.points_from_pairs()
        b.pair_weight_grads()
        b.block1_point_half()
        if plan.xyz:
            b.xyz()
        return b.outputs()


class _BwdPlan(NamedTuple):
    """Every decision of one AggregateFn.backward, made once."""
    n: int               # valid sample rows (read from the counts when the forward ran on device counts)
    used: Any            # the referenced rows, cut to their count; None: block1.0's point half over the whole table
    chain: str           # the per-pair dX chain: "fp32" | "x3" | "h2" (_PAIRS)
    gemm: str            # the weight-gradient and colour-branch GEMMs: "x3" | "h2"
    point_extras: bool   # d colour / d dir wanted: block3.0's extras per point (pnr_pairs_to_points_ex)
    xyz: bool            # d xyz wanted
    native: bool         # the whole backward as pnr_aggregate_bwd_step_h2

    @property
    def n_used(self):
        return None if self.used is None else self.used.numel()

    @classmethod
    def of(cls, ctx):
        spec = ctx.spec
        n, used = spec.n, None if spec.used is None else spec.used.rows
        if spec.counts is not None:   # the forward ran on device counts: read them now (no drain)
            cnt = spec.counts.get()
            n = cnt["S_valid"]
            if used is not None:
                used = used[:cnt["n_used"]]
        # the forward's precision picks the chain; fp32h2 runs it on f16 splits unless BWD_H2 is off
        chain = {"fp32": "fp32", "fp32x3": "x3", "fp32h2": "h2" if BWD_H2 else "x3"}[spec.precision]
        # fp32 has no GEMM kernels of its own here: its weight gradients run on pnr_gemm_tn_x3
        # (fp32-accurate) like fp32x3's, its dX products on pnr_gemm_nn (exact fp32)
        gemm = "h2" if spec.precision == "fp32h2" else "x3"
        has_c, has_d, _ = ctx.has
        xyz = ctx.xyz_shape is not None and ctx.needs_input_grad[5]
        # (a pair mask cannot come with a split chain: AggSpec refuses it)
        native = NATIVE_BWD and chain == "h2" and used is not None and not xyz
        # d colour / d dir never come from the pairs pass (its float atomics made the fp32
        # chain's differ from run to run): every chain sums them per point in pair order
        return cls(n, used, chain, gemm, has_c or has_d, xyz, native)


# chain -> entry point; the split chains take their split packs after the pnr_mlp_bwd
_PAIRS = {"fp32": "pnr_aggregate_bwd_pairs", "x3": "pnr_aggregate_bwd_pairs_x3", "h2": "pnr_aggregate_bwd_pairs_h2"}


class _Backward:
    """AggregateFn.backward as the Python sequence: the stages in the order of the
    kernels, which is the order of pnr_aggregate_bwd_step_h2 (csrc/train_step.hip).

    Buffers: what a kernel writes in full is ``empty``; what it accumulates into,
    or writes only the referenced rows of, is ``zeros`` -- the full-table outputs
    d emb / d colour / d dir / d conf / d xyz, the padded GEMM operands, and d_p1
    without a used-point list."""

    def __init__(self, ctx, d_feat, plan: _BwdPlan):
        self.ctx, self.spec, self.sv, self.plan, self.d_feat = ctx, ctx.spec, ctx.sv, plan, d_feat
        self.P = dict(zip(_PARAM_NAMES, ctx.saved_tensors))
        self.dev = d_feat.device
        self.f32 = dict(dtype=torch.float32, device=self.dev)
        self.slope = float(ctx.spec.agg.neg_slope)
        self.N = ctx.tabs[0].shape[0]
        self.n_p1 = self.N if plan.used is None else plan.used.numel()   # rows of block1.0's point half
        self.m = plan.n * 8                                                # pairs
        # fp32h2: the GEMMs on the f16-split kernels (pnr_gemm_*_h2), fp32x3 / fp32 on the bf16x3 ones
        self.hg = L.H2Gemm(self.dev) if plan.gemm == "h2" else None
        self.grads = {}
        self.d_xyz = None

    def _refs(self):
        ctx = self.ctx
        return ctypes.byref(ctx.pts), ctypes.byref(self.spec.samples), ctypes.byref(ctx.mlp)

    def _gemm_tn(self, dz, x, am, colsum=False):
        return L.gemm_tn(dz, x, colsum=colsum, h2=self.hg, a_absmax=am)

    def colour_branch(self):
        """color_branch.{0,2,4}: 280 -> 128 -> 128 -> 128, LeakyReLU each.  dZ's scale
        for the f16-split kernels: fused into pnr_color_dz, then one pnr_absmax pass
        per layer (the colour batch is ~30 k rows)."""
        sv, hg, P, grads, f32, n, slope = self.sv, self.hg, self.P, self.grads, self.f32, self.plan.n, self.slope
        d_feat, dev = self.d_feat, self.dev
        hc1, hc2, hc3 = sv["hc1"][:n], sv["hc2"][:n], sv["hc3"][:n]

        def amax(t):
            return hg.absmax(t) if hg is not None and t.shape[0] > 0 else None

        # dz = lrelu'(hc3) (d_feat[:, 1:] * vmask) and its max |.| in one pass
        dz = torch.empty((n, 128), **f32)
        am = hg.words[1:2] if hg is not None and n > 0 else None
        L.check(L.lib().pnr_color_dz(L.ptr(d_feat), d_feat.stride(0), L.ptr(sv["vmask"]), L.ptr(hc3), hc3.stride(0),
                                     n, 128, slope, L.ptr(dz), L.ptr(am), L.stream_ptr(dev)), "pnr_color_dz")
        grads["color_branch.4.weight"], grads["color_branch.4.bias"] = self._gemm_tn(dz, hc2.contiguous(), am, True)
        dz = L.gemm_nn(dz, P["color_branch.4.weight"], act=hc2, slope=slope, h2=hg, a_absmax=am)
        am = amax(dz)
        grads["color_branch.2.weight"], grads["color_branch.2.bias"] = self._gemm_tn(dz, hc1.contiguous(), am, True)
        dz = L.gemm_nn(dz, P["color_branch.2.weight"], act=hc1, slope=slope, h2=hg, a_absmax=am)
        am = amax(dz)
        gC0 = torch.empty((128, 280), **f32)
        gC0[:, :256], grads["color_branch.0.bias"] = self._gemm_tn(dz, sv["hid"][:n], am, True)
        vpe32 = torch.zeros((n, 32), **f32)           # K padded to the GEMM's 32-column tiles
        vpe32[:, :24] = sv["vpe"][:n]
        gC0[:, 256:] = self._gemm_tn(dz, vpe32, am)[:, :24]
        grads["color_branch.0.weight"] = gC0
        self.d_hid = torch.empty((max(n, 1), 256), **f32)   # rows [0, n) written by the gemm_nn
        L.gemm_nn(dz, P["color_branch.0.weight"][:, :256], out=self.d_hid[:n], h2=hg, a_absmax=am)

    def pairs_chain(self):
        """The per-pair dX chain on MFMA: dz1..dz4 and d alpha-pre-activation per pair,
        the per-pair d conf terms."""
        plan, f32, N = self.plan, self.f32, self.N
        has_c, has_d, has_f = self.ctx.has
        Pn = max(plan.n, 1) * 8
        self.dz = [torch.empty((Pn, 256), **f32) for _ in range(4)]
        self.dpa = torch.empty(Pn, **f32)
        # pnr_pairs_to_points writes the row of every point some pair references: every
        # row of a used-point list, only some of the whole table's
        self.d_p1 = (torch.empty if plan.used is not None else torch.zeros)((max(self.n_p1, 1), 256), **f32)
        self.d_color = torch.zeros((N, 3), **f32) if has_c else None
        self.d_dir = torch.zeros((N, 3), **f32) if has_d else None
        self.d_conf = torch.zeros(N, **f32) if has_f else None
        # the pairs' d conf terms, written per pair and summed per point in pair order by
        # pnr_pairs_to_points_conf (no float atomics: bitwise repeatable)
        self.dconf_pair = torch.empty(Pn, **f32) if has_f else None
        # the block3.0 extras' colour / dir gradients are made per point in points_from_pairs
        # (no float atomics): the pairs pass gets no d colour / d dir, and no w3e either --
        # except the fp32 kernel, which wants it bound
        self.packs = pk = packed_bwd(self.spec.agg, plan.chain, pairs_w3e=plan.chain == "fp32")
        split = () if pk.split is None else (ctypes.byref(pk.split),)
        # d_p1 = NULL: the per-point sums of dz1 come from pnr_pairs_to_points (pairs
        # sorted by point: no atomics, deterministic) instead of the kernel's atomics
        entry = _PAIRS[plan.chain]
        L.check(getattr(L.lib(), entry)(*self._refs(), ctypes.byref(pk.mlp), *split, ctypes.byref(self.sv.c),
                                        L.ptr(self.d_feat), L.ptr(self.d_hid), *(L.ptr(t) for t in self.dz),
                                        L.ptr(self.dpa), None, None, None, L.ptr(self.dconf_pair),
                                        L.stream_ptr(self.dev)), entry)

    def points_from_pairs(self):
        """The pairs grouped by point in pair order (torch.sort(prow, stable=True)
        natively), then each point's sums: d conf, d P1 and the extras' d colour / d dir."""
        ctx, sv, plan, m, dev = self.ctx, self.sv, self.plan, self.m, self.dev
        row_map = None if self.spec.used is None else self.spec.used.row_map
        prow_sorted, pair_of = L.group_pairs(sv["prow"][:m], row_map, self.n_p1)
        if self.d_conf is not None:
            L.check(L.lib().pnr_pairs_to_points_conf(L.ptr(prow_sorted), L.ptr(pair_of), m, L.ptr(self.dconf_pair),
                                                     L.ptr(self.d_conf), L.stream_ptr(dev)), "pnr_pairs_to_points_conf")
        dz1, dz3 = self.dz[0], self.dz[2]
        if plan.point_extras:
            g_pair = torch.empty((max(m, 1), 8), **self.f32)
            L.check(L.lib().pnr_aggregate_bwd_extras_rows(*self._refs(), ctypes.byref(sv.c), L.ptr(self.packs.w3e),
                                                          L.ptr(dz3), L.ptr(g_pair), L.stream_ptr(dev)),
                    "pnr_aggregate_bwd_extras_rows")
            L.check(L.lib().pnr_pairs_to_points_ex(L.ptr(prow_sorted), L.ptr(pair_of), m, L.ptr(dz1), L.ptr(row_map),
                                                   L.ptr(self.d_p1), L.ptr(sv.absmax(5)), L.ptr(g_pair),
                                                   L.c_void_p(ctx.mlp.rw2c or None), L.c_void_p(ctx.pts.rw2c or None),
                                                   L.ptr(self.d_color), L.ptr(self.d_dir), L.stream_ptr(dev)),
                    "pnr_pairs_to_points_ex")
        else:
            L.check(L.lib().pnr_pairs_to_points(L.ptr(prow_sorted), L.ptr(pair_of), m, L.ptr(dz1), L.ptr(row_map),
                                                L.ptr(self.d_p1), L.ptr(sv.absmax(5)), L.stream_ptr(dev)),
                    "pnr_pairs_to_points")

    def pair_weight_grads(self):
        """dW = dZ^T X over all pairs: split-K MFMA GEMMs, bias = column sums.  The A
        operands' scales: the maxima k_pairs_bwd wrote (no extra pass)."""
        sv, grads, m, f32, amx = self.sv, self.grads, self.m, self.f32, self.sv.absmax
        _, dz2, dz3, dz4 = (t[:m] for t in self.dz)
        dpa = self.dpa[:m]
        h1, h2, h3, h4 = sv["h1"][:m], sv["h2"][:m], sv["h3"][:m], sv["h4"][:m]
        grads["block3.2.weight"], grads["block3.2.bias"] = self._gemm_tn(dz4, h3, amx(3), True)
        gW3 = torch.empty((256, 263), **f32)
        gW3[:, :256], grads["block3.0.bias"] = self._gemm_tn(dz3, h2, amx(2), True)
        gW3[:, 256:] = self._gemm_tn(dz3, sv["x3e"][:m], amx(2))[:, :7]
        grads["block3.0.weight"] = gW3
        grads["block1.2.weight"], grads["block1.2.bias"] = self._gemm_tn(dz2, h1, amx(1), True)
        dpa32 = torch.zeros((m, 32), **f32)      # M padded to one 32-row MFMA tile
        dpa32[:, 0] = dpa
        grads["alpha_branch.0.weight"] = self._gemm_tn(dpa32, h4, amx(4))[:1]
        grads["alpha_branch.0.bias"] = dpa.sum(0, keepdim=True)

    def block1_point_half(self):
        """block1.0: the point half from d P1 and X1 = [emb, PE_3(emb)], the pair half
        from dz1 and PE_5; then d emb through PE_3's backward."""
        sv, hg, grads, m, f32, dev = self.sv, self.hg, self.grads, self.m, self.f32, self.dev
        used, n_p1, amx = self.plan.used, self.n_p1, self.sv.absmax
        emb = self.ctx.tabs[0]
        dz1 = self.dz[0][:m]
        d_p1 = self.d_p1[:n_p1]
        if sv["x1"] is not None:   # the forward's rows (k_point_pre_h2: fp32h2 with a used-point list)
            x1 = sv["x1"][:n_p1]
        else:
            x1 = torch.empty((max(n_p1, 1), 224), **f32)[:n_p1]
            if used is None:
                L.check(L.lib().pnr_point_pe3(L.ptr(emb), n_p1, L.ptr(x1), L.stream_ptr(dev)), "pnr_point_pe3")
            else:   # PE_3 of the used rows, read through the list (no gathered copy)
                L.check(L.lib().pnr_point_pe3_rows(L.ptr(emb), L.ptr(used), n_p1, L.ptr(x1), L.stream_ptr(dev)),
                        "pnr_point_pe3_rows")
        gW1 = torch.empty((256, 284), **f32)
        gW1[:, :224], grads["block1.0.bias"] = self._gemm_tn(d_p1, x1, amx(5), True)   # sum_p dP1 = sum_pairs dz1
        gW1[:, 224:] = self._gemm_tn(dz1, sv["pe5"][:m], amx(0))[:, :60]
        grads["block1.0.weight"] = gW1
        dx1 = L.gemm_nn(d_p1, self.P["block1.0.weight"][:, :224], h2=hg, a_absmax=amx(5))
        self.d_emb = torch.zeros((self.N, 32), **f32)
        if used is None:
            L.check(L.lib().pnr_point_pe3_bwd(L.ptr(emb), L.ptr(dx1), n_p1, L.ptr(self.d_emb), L.stream_ptr(dev)),
                    "pnr_point_pe3_bwd")
        else:   # straight into the used rows of the full gradient (no index_copy)
            L.check(L.lib().pnr_point_pe3_bwd_rows(L.ptr(emb), L.ptr(used), L.ptr(dx1), n_p1, L.ptr(self.d_emb),
                                                   L.stream_ptr(dev)), "pnr_point_pe3_bwd_rows")

    def xyz(self):
        """d PE_5 = dz1 . W1[:, 224:284], then the distance / weight / w2pers chain per pair."""
        f32 = self.f32
        d_xyz = torch.zeros((self.N, 3), **f32)
        if self.m > 0:   # (an empty list has no d PE_5 rows to hand over: d xyz stays 0)
            w1pe = torch.zeros((256, 64), **f32)          # N padded to the GEMM's 32-column tiles
            w1pe[:, :60] = self.P["block1.0.weight"][:, 224:284]
            d_pe = L.gemm_nn(self.dz[0][:self.m], w1pe)
            L.check(L.lib().pnr_aggregate_bwd_xyz(*self._refs(), ctypes.byref(self.sv.c), L.ptr(self.d_feat),
                                                  L.ptr(self.d_hid), L.ptr(d_pe), L.ptr(d_xyz),
                                                  L.stream_ptr(self.dev)), "pnr_aggregate_bwd_xyz")
        self.d_xyz = d_xyz.view(self.ctx.xyz_shape)

    def outputs(self) -> tuple:
        emb_shape, conf_shape = self.ctx.shapes
        d_conf = None if self.d_conf is None else self.d_conf.view(conf_shape)
        return (None, self.d_emb.view(emb_shape), self.d_color, self.d_dir, d_conf, self.d_xyz,
                *(self.grads[k] for k in _PARAM_NAMES))


def _native_bwd_h2(ctx, spec, d_feat, n: int, n_used: int, params) -> tuple:
    """AggregateFn.backward for fp32h2 through pnr_aggregate_bwd_step_h2: every
    gradient in one host call (outputs allocated here, written by the step)."""
    dev = d_feat.device
    N = ctx.tabs[0].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    prm, out = L.AggParams(), L.AggGrads()
    grads = []
    for i, p in enumerate(params):
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise L.PnrError(f"native backward: parameter {_PARAM_NAMES[i]} must be contiguous fp32")
        prm.p[i] = p.data_ptr()
        grads.append(torch.empty(p.shape, **f32))
        out.g[i] = grads[-1].data_ptr()
    has_c, has_d, has_f = ctx.has
    d_emb = torch.empty((N, 32), **f32)
    d_color = torch.empty((N, 3), **f32) if has_c else None
    d_dir = torch.empty((N, 3), **f32) if has_d else None
    d_conf = torch.empty(N, **f32) if has_f else None
    out.d_emb, out.d_color, out.d_dir, out.d_conf = (None if t is None else t.data_ptr()
                                                     for t in (d_emb, d_color, d_dir, d_conf))
    scratch = L.scratch("pnr_aggregate_bwd_step_h2_scratch_bytes", n, n_used, device=dev)
    L.check(L.lib().pnr_aggregate_bwd_step_h2(ctypes.byref(ctx.pts), ctypes.byref(spec.samples),
                                              ctypes.byref(ctx.mlp), ctypes.byref(prm), ctypes.byref(ctx.sv.c),
                                              L.ptr(d_feat), n, n_used, ctypes.byref(out), L.ptr(scratch),
                                              scratch.numel(), L.stream_ptr(dev)), "pnr_aggregate_bwd_step_h2")
    emb_shape, conf_shape = ctx.shapes
    return (None, d_emb.view(emb_shape), d_color, d_dir, None if d_conf is None else d_conf.view(conf_shape),
            None, *grads)


class RgbHeadFn(torch.autograd.Function):
    """[n, 4] = [feat[:, 0], raw2out_color(feat[:, 1:] W^T + b)] -- the upstream
    colour head (point_aggregators.py:343, 269-273, 637-638) on pnr_rgb_head_fwd,
    backward on pnr_rgb_head_bwd (d feat, d W, d b)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, act_super, n_dev, n):
        dev = feat.device
        f = feat.detach().contiguous()
        w, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        out = torch.zeros((max(f.shape[0], 1), 4), dtype=torch.float32, device=dev)[:f.shape[0]]
        L.check(L.lib().pnr_rgb_head_fwd(L.ptr(f), f.stride(0), L.ptr(n_dev), int(n), L.ptr(w), L.ptr(b),
                                         int(act_super), L.ptr(out), L.stream_ptr(dev)), "pnr_rgb_head_fwd")
        ctx.f, ctx.w, ctx.b, ctx.act, ctx.n_dev, ctx.n = f, w, b, int(act_super), n_dev, int(n)
        return out

    @staticmethod
    def backward(ctx, d_out):
        dev = d_out.device
        d_out = d_out.contiguous()
        d_feat = torch.zeros_like(ctx.f)
        d_wb = torch.empty((3, 129), dtype=torch.float32, device=dev)
        partials = torch.empty((L.HEAD_BWD_BLOCKS, 3, 129), dtype=torch.float32, device=dev)
        L.check(L.lib().pnr_rgb_head_bwd(L.ptr(d_out), L.ptr(ctx.f), ctx.f.stride(0), L.ptr(ctx.n_dev), ctx.n,
                                         L.ptr(ctx.w), L.ptr(ctx.b), ctx.act, L.ptr(d_feat), L.ptr(d_wb),
                                         L.ptr(partials), L.stream_ptr(dev)), "pnr_rgb_head_bwd")
        return d_feat, d_wb[:, :128].contiguous(), d_wb[:, 128].contiguous(), None, None, None


class CompositeSpec:
    def __init__(self, rays, qp, bufs, cp, R, SR, C, keep=(), counts=None):
        self.rays, self.qp, self.bufs, self.cp = rays, qp, bufs, cp
        self.R, self.SR, self.C = R, SR, C
        self.keep = keep
        self.counts = counts   # set: feat is capacity-sized, its rows counted on the device (counts[1])


class CompositeFn(torch.autograd.Function):
    """ray_color[R, C] = composite(feat[S_valid, C+1], bg[C]); opacity / is_bg /
    mask are returned as non-differentiable outputs.  bg (optional) is the
    learned background colour (mvs_points_volumetric_model.py:92-94): its
    gradient is sum_r is_bg[r] d ray_color[r] -- bg_T for a hit ray (the
    ray_march term, diff_ray_marching.py:544-546), 1 for a background ray
    (fill_invalid, neural_points_volumetric_model.py:373-375) -- on
    pnr_weighted_colsum."""

    @staticmethod
    def forward(ctx, spec: CompositeSpec, feat, bg=None):
        dev = feat.device
        f32 = dict(dtype=torch.float32, device=dev)
        R, SR, C = spec.R, spec.SR, spec.C
        ray_color = torch.empty((R, C), **f32)
        opacity = torch.empty((R, SR), **f32)
        is_bg = torch.empty((R,), **f32)
        ray_mask = torch.empty((R,), dtype=torch.int8, device=dev)
        feat_c = feat.detach().contiguous()
        bg_c = None if bg is None else bg.detach().float().reshape(-1).contiguous()
        spec.cp.bg_color = L.ptr(bg_c)
        L.check(L.lib().pnr_composite_fwd(ctypes.byref(spec.rays), ctypes.byref(spec.qp), ctypes.byref(spec.bufs.c),
                                          ctypes.byref(spec.cp), L.ptr(feat_c), L.ptr(ray_color), L.ptr(opacity),
                                          L.ptr(is_bg), L.ptr(ray_mask), L.stream_ptr(dev)),
                "pnr_composite_fwd")
        ctx.spec, ctx.feat, ctx.bg, ctx.is_bg = spec, feat_c, bg_c, is_bg
        ctx.mark_non_differentiable(opacity, is_bg, ray_mask)
        return ray_color, opacity, is_bg, ray_mask

    @staticmethod
    def backward(ctx, d_color, _d_op, _d_bg, _d_mask):
        spec = ctx.spec
        dev = ctx.feat.device
        if spec.counts is not None and ctx.feat.dim() == 2:   # zero only the device-counted rows
            d_feat = _rows_zeroed(tuple(ctx.feat.shape), spec.bufs.count_ptr(COUNT_S_VALID), dev)
        else:
            d_feat = torch.zeros_like(ctx.feat)
        if d_color is None:
            return None, d_feat, None
        d_color = d_color.contiguous()
        spec.cp.bg_color = L.ptr(ctx.bg)
        L.check(L.lib().pnr_composite_bwd(ctypes.byref(spec.rays), ctypes.byref(spec.qp), ctypes.byref(spec.bufs.c),
                                          ctypes.byref(spec.cp), L.ptr(ctx.feat), L.ptr(d_color), L.ptr(d_feat),
                                          L.stream_ptr(dev)),
                "pnr_composite_bwd")
        d_bg = None
        if ctx.bg is not None and ctx.needs_input_grad[2]:
            d_bg = L.weighted_colsum(ctx.is_bg, d_color)
        return None, d_feat, d_bg


def ray_march_bwd(ray_dist, ray_valid, feat, bg, d_color):
    """d feat of pnr_ray_march_fwd (dense mirror) for a given d ray_color."""
    NR, SR, CF = feat.shape
    d_feat = torch.zeros_like(feat)
    L.check(L.lib().pnr_ray_march_bwd(L.ptr(ray_dist), L.ptr(ray_valid), L.ptr(feat), L.ptr(bg), NR, SR, CF - 1,
                                      L.ptr(d_color.contiguous()), L.ptr(d_feat), L.stream_ptr(feat.device)),
            "pnr_ray_march_bwd")
    return d_feat
