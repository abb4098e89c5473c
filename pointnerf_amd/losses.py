"""The finetune objective of the reference on libpnr, without a host read.

``compute_losses`` (models/base_rendering_model.py:533-664) selects the hit /
missed rays with ``torch.masked_select`` and branches in Python on how many
there are: a device drain per tensor.  Here the colour items of one output
tensor come from one kernel pass (``pnr_color_loss_fwd``: all four kinds and
their ray counts, on the device) with a one-launch backward, and the sparse
loss is computed per point from the query buffers of the last
``render_rays_train`` (``pnr_sparse_loss_fwd``).  Same values and gradients as
the reference's formulation, bitwise repeatable.  See DESIGN.md "Objective".

  color_losses(x, gt, ray_mask, extra_mask=None) -> (values [4], counts [4])
  RenderLoss(opt)(output, gt_image, model=None, ray_depth_mask=None) -> (loss_total, dict)
  frame_metrics(output, gt_image, items) -> dict
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L
from .querier import COUNT_R_VALID

# item-name prefixes of compute_losses (:543, :552, :564) -> index into color_losses' values
PLAIN, MASKED, MISS, DEPTH_MASKED = 0, 1, 2, 3
KINDS = (("ray_masked_", MASKED), ("ray_miss_", MISS), ("ray_depth_masked_", DEPTH_MASKED))


def split_item(name: str):
    """'ray_masked_coarse_raycolor' -> (1, 'coarse_raycolor'); no prefix -> (0, name)."""
    for prefix, kind in KINDS:
        if name.startswith(prefix):
            return kind, name[len(prefix):]
    if name.startswith("ray_"):
        raise L.PnrError(f"colour loss item {name!r}: unknown kind (plain, ray_masked_, ray_miss_ or "
                         "ray_depth_masked_)")
    return PLAIN, name


def _rows(t: torch.Tensor, what: str):
    """[..., C] float tensor as a [R, C] view with unit channel stride and one
    row stride (a copy only when the layout has none)."""
    if t.dim() < 1:
        raise L.PnrError(f"{what}: expected [..., C], got a scalar")
    t2 = t.reshape(-1, t.shape[-1])
    if t2.dtype != torch.float32:
        t2 = t2.float()
    if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]):
        t2 = t2.contiguous()
    return t2


def _ld(t2: torch.Tensor) -> int:
    return int(t2.stride(0)) if t2.shape[0] > 1 else int(t2.shape[1])


class _ColorLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gt, ray_mask, extra_mask):
        L.require_gpu(x)
        dev = x.device
        x2 = _rows(x.detach(), "color_losses x")
        g2 = _rows(gt.detach().to(dev), "color_losses gt")
        R, C = x2.shape
        if tuple(g2.shape) != (R, C):
            raise L.PnrError(f"color_losses: x is [{R},{C}], gt is {list(g2.shape)}")
        rm = ray_mask.detach().reshape(-1)
        if rm.dtype != torch.int8:
            rm = rm.to(torch.int8)
        rm = rm.contiguous()
        if rm.numel() != R:
            raise L.PnrError(f"color_losses: ray_mask holds {rm.numel()} rays, x {R}")
        em = None
        if extra_mask is not None:
            em = extra_mask.detach().reshape(-1)
            em = (em > 0).to(torch.uint8) if em.dtype != torch.uint8 else em.contiguous()
            if em.numel() != R:
                raise L.PnrError(f"color_losses: extra_mask holds {em.numel()} rays, x {R}")
        out = torch.empty(4, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        scratch = L.scratch("pnr_color_loss_scratch_bytes", device=dev)
        L.check(L.lib().pnr_color_loss_fwd(L.ptr(x2), _ld(x2), L.ptr(g2), _ld(g2), L.ptr(rm), L.ptr(em), R, C,
                                           L.ptr(out), L.ptr(counts), L.ptr(scratch), scratch.numel(),
                                           L.stream_ptr(dev)),
                "pnr_color_loss_fwd")
        ctx.save_for_backward(x2, g2, rm, counts)
        ctx.em = em
        ctx.x_shape = x.shape
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    def backward(ctx, g_out, _g_counts):
        x2, g2, rm, counts = ctx.saved_tensors
        R, C = x2.shape
        dev = x2.device
        g = g_out.reshape(4).float().contiguous()
        d = torch.empty((R, C), dtype=torch.float32, device=dev)
        L.check(L.lib().pnr_color_loss_bwd(L.ptr(x2), _ld(x2), L.ptr(g2), _ld(g2), L.ptr(rm), L.ptr(ctx.em), R, C,
                                           L.ptr(counts), L.ptr(g), L.ptr(d), C, L.stream_ptr(dev)),
                "pnr_color_loss_bwd")
        return d.reshape(ctx.x_shape), None, None, None


def color_losses(x, gt, ray_mask, extra_mask=None):
    """The four colour-item kinds of compute_losses for one output tensor
    x [..., C] against gt [..., C], with ray_mask [R] (the output dict's
    ``ray_mask``) and an optional per-ray extra_mask [R] (ray_depth_masked_):

      values[0]  MSE over every ray                       (``coarse_raycolor``)
      values[1]  MSE over the rays with ray_mask > 0      (``ray_masked_*``), 0 when there is none
      values[2]  MSE over ray_mask == 0 x their number    (``ray_miss_*``),   0 when there is none
      values[3]  MSE over extra_mask > 0                  (``ray_depth_masked_*``), 0 when empty

    and counts [4] int64 = (R, hit, missed, extra rays), both on the device.
    Differentiable in x (one launch); C <= 128; x may be a strided view such as
    color[:, :3].  Bitwise repeatable, no host read."""
    return _ColorLosses.apply(x, gt, ray_mask, extra_mask)


class _SparseConfLoss(torch.autograd.Function):
    """NeuralPointsRayMarching.sparse_conf_loss on libpnr (pnr_sparse_loss_fwd /
    _bwd): per-point summed pair weights in fixed point, one reduction, one
    backward kernel; no host read and no [1, R'', SR, K] tensors."""

    @staticmethod
    def forward(ctx, conf, xyz, bufs, qp):
        dev = xyz.device
        N = xyz.shape[0]
        c = None if conf is None else conf.detach().float().reshape(-1).contiguous()
        wfix = torch.empty(N, dtype=torch.int64, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        state = torch.empty(1, dtype=torch.float64, device=dev)
        scratch = L.scratch("pnr_sparse_loss_scratch_bytes", device=dev)
        L.check(L.lib().pnr_sparse_loss_fwd(ctypes.byref(qp), ctypes.byref(bufs.c), bufs.R, L.ptr(xyz), L.ptr(c), N,
                                            L.ptr(wfix), L.ptr(out), L.ptr(state), L.ptr(scratch), scratch.numel(),
                                            L.stream_ptr(dev)), "pnr_sparse_loss_fwd")
        if c is not None:
            ctx.save_for_backward(c, wfix, state)
        ctx.conf_shape = None if conf is None else conf.shape
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        c, wfix, state = ctx.saved_tensors
        d = torch.empty_like(c)
        g = g.reshape(1).float().contiguous()
        L.check(L.lib().pnr_sparse_loss_bwd(L.ptr(wfix), L.ptr(c), c.numel(), L.ptr(state), L.ptr(g), L.ptr(d),
                                            L.stream_ptr(c.device)), "pnr_sparse_loss_bwd")
        return d.reshape(ctx.conf_shape), None, None, None


class _ZeroOneConfLoss(torch.autograd.Function):
    """NeuralPointsRayMarching.zero_one_conf_loss on libpnr: the per-point entry
    counts of the query's neighbour lists (pnr_point_counts), then one fused
    reduction (pnr_zero_one_loss_fwd) and one backward kernel -- the same value
    and gradient as torch's clamp / log / mean over the gathered [1, R'', SR, K]
    conf_coefficient, in three launches and without host reads."""

    @staticmethod
    def forward(ctx, conf, bufs, SR, K, eps):
        dev = conf.device
        N = conf.numel()
        c = conf.detach().float().contiguous()
        counts = torch.zeros(N, dtype=torch.float32, device=dev)
        L.check(L.lib().pnr_point_counts(L.ptr(bufs.pidx), L.ptr(bufs.counts), K, bufs.pidx.numel() // K,
                                         L.ptr(counts), L.stream_ptr(dev)), "pnr_point_counts")
        part = torch.empty(1024, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        L.check(L.lib().pnr_zero_one_loss_fwd(L.ptr(c), L.ptr(counts), N, L.c_void_p(bufs.count_ptr(COUNT_R_VALID)),
                                              SR * K, eps, L.ptr(part), L.ptr(out), L.stream_ptr(dev)),
                "pnr_zero_one_loss_fwd")
        ctx.save_for_backward(c, counts, out)
        ctx.eps = eps
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        c, counts, out = ctx.saved_tensors
        d = torch.empty_like(c)
        g = g.reshape(1).float().contiguous()
        L.check(L.lib().pnr_zero_one_loss_bwd(L.ptr(c), L.ptr(counts), c.numel(), ctx.eps, L.ptr(out), L.ptr(g),
                                              L.ptr(d), L.stream_ptr(c.device)), "pnr_zero_one_loss_bwd")
        return d, None, None, None, None


def sparse_loss(weight, conf_coefficient):
    """base_rendering_model.py:657 on the output dict's tensors (the path for
    callers without a model; NeuralPointsRayMarching.sparse_conf_loss is the
    native one)."""
    cc = conf_coefficient if torch.is_tensor(conf_coefficient) else \
        torch.as_tensor(float(conf_coefficient), device=weight.device)
    return torch.sum(weight * torch.abs(1 - torch.exp(-2 * cc))) / (torch.sum(weight) + 1e-6)


def mse2psnr(x):
    """-10 log10(x) (base_rendering_model.py:17) on the device: taken in fp64
    and rounded to fp32 once."""
    return (torch.log(x.double()) * (-10.0 / math.log(10.0))).to(x.dtype)


def _weights(w, n: int, what: str):
    """One weight broadcasts to every item (check_setup_loss, :227-234)."""
    w = [float(v) for v in (w if isinstance(w, (list, tuple)) or hasattr(w, "__len__") else [w])]
    if len(w) == 1 and n > 1:
        w = w * n
    if len(w) != n:
        raise L.PnrError(f"{what}: {len(w)} weights for {n} items (one weight, or one per item)")
    return w


def _output(output, key, what):
    if key not in output:
        raise L.PnrError(f"{what}: the output dict has no {key!r} (keys: {sorted(output)})")
    return output[key]


def _color_passes(output, gt_image, items, ray_depth_mask):
    """One color_losses pass per distinct output tensor the items name:
    ([values [4] per tensor], {item name: (pass index, kind)})."""
    order, where = [], {}
    for name in items:
        kind, key = split_item(name)
        if key not in order:
            order.append(key)
        where[name] = (order.index(key), kind)
    passes = []
    for i, key in enumerate(order):
        x = _output(output, key, "colour loss item")
        if x.shape[-1] != gt_image.shape[-1]:
            raise L.PnrError(f"colour loss on {key!r}: the output has {x.shape[-1]} channels, gt_image "
                             f"{gt_image.shape[-1]} (render with C_out = {gt_image.shape[-1]} or slice the output)")
        extra = None
        if any(p == i and kind == DEPTH_MASKED for p, kind in where.values()):
            if ray_depth_mask is None:
                raise L.PnrError("a ray_depth_masked_ item needs ray_depth_mask (the per-ray mask, "
                                 "base_rendering_model.py:565-566)")
            extra = ray_depth_mask
        passes.append(color_losses(x, gt_image, _output(output, "ray_mask", "colour loss item"), extra)[0])
    return passes, where


class RenderLoss:
    """compute_losses (base_rendering_model.py:533-664) for a model of this
    package: ``RenderLoss(opt)(output, gt_image, model=None, ray_depth_mask=None)``
    returns (loss_total, {"loss_<name>": value, "psnr_<name>": value}), all
    device tensors; nothing is read on the host.

    Reads opt.color_loss_items / color_loss_weights (loss * weight + 1e-6 per
    item, :603), opt.zero_one_loss_items / zero_one_loss_weights / zero_epsilon
    (item "conf_coefficient": model.zero_one_conf_loss() when a model is given,
    else zero_one_loss on the dict entry) and opt.sparse_loss_weight
    (model.sparse_conf_loss(), else :657 on output["weight"] and
    ["conf_coefficient"]).  Depth, background and l2-size items are refused.

    loss_total is the weighted sum of the fp32 item values taken in fp64 (one
    dot product with a cached device weight vector) and rounded to fp32 once."""

    def __init__(self, opt):
        self.opt = opt
        self.color_items = list(getattr(opt, "color_loss_items", None) or [])
        self.color_weights = _weights(getattr(opt, "color_loss_weights", [1.0]), len(self.color_items),
                                      "color_loss_weights") if self.color_items else []
        for name in self.color_items:
            split_item(name)
        for group in ("depth_loss_items", "bg_loss_items", "l2_size_loss_items"):
            if getattr(opt, group, None):
                raise L.PnrError(f"{group} = {list(getattr(opt, group))}: not implemented (colour, zero-one and "
                                 "sparse losses only)")
        self.zero_one_items = list(getattr(opt, "zero_one_loss_items", None) or [])
        self.zero_one_weights = _weights(getattr(opt, "zero_one_loss_weights", [1.0]), len(self.zero_one_items),
                                         "zero_one_loss_weights") if self.zero_one_items else []
        self.zero_epsilon = float(getattr(opt, "zero_epsilon", 1e-3))
        self.sparse_weight = float(getattr(opt, "sparse_loss_weight", 0) or 0)
        self._wvec = {}

    def _weight_vector(self, w, dev):
        """The term weights as a device fp64 vector, uploaded once per device
        from pinned memory (no stream wait)."""
        key = (str(dev), tuple(w))
        if key not in self._wvec:
            t = torch.tensor(w, dtype=torch.float64)
            self._wvec[key] = t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)
        return self._wvec[key]

    def __call__(self, output, gt_image, model=None, ray_depth_mask=None):
        from .renderer import NeuralPointsRayMarching
        losses = {}
        passes, where = _color_passes(output, gt_image, self.color_items, ray_depth_mask)
        parts = list(passes)                      # 1-D fp32 tensors, concatenated below
        w = [0.0] * (4 * len(passes))             # their weights, in the same order
        psnr = [mse2psnr(v.detach()) for v in passes]
        for name, wi in zip(self.color_items, self.color_weights):
            p, kind = where[name]
            w[4 * p + kind] += wi
            losses["loss_" + name] = passes[p][kind]
            losses["psnr_" + name] = psnr[p][kind]
        const = 1e-6 * len(self.color_items)      # + 1e-6 per colour item (:603)
        for name, wi in zip(self.zero_one_items, self.zero_one_weights):
            if model is not None and name == "conf_coefficient" and model.neural_points.points_conf is not None:
                loss = model.zero_one_conf_loss(self.zero_epsilon)
            else:
                val = _output(output, name, "zero_one loss item")
                if not torch.is_tensor(val):
                    continue   # a cloud without a conf table: conf_coefficient is the constant 1, no term
                loss = NeuralPointsRayMarching.zero_one_loss(val, self.zero_epsilon)
            parts.append(loss.reshape(1))
            w.append(wi)
            losses["loss_" + name] = loss
        if self.sparse_weight > 0:
            if model is not None:
                loss = model.sparse_conf_loss()
            else:
                loss = sparse_loss(_output(output, "weight", "sparse loss"),
                                   _output(output, "conf_coefficient", "sparse loss"))
            parts.append(loss.reshape(1))
            w.append(self.sparse_weight)
            losses["loss_sparse"] = loss
        if not parts:
            raise L.PnrError("RenderLoss: no loss item is configured")
        flat = parts[0] if len(parts) == 1 else torch.cat([p.float() for p in parts])
        total = (torch.dot(flat.double(), self._weight_vector(w, flat.device)) + const).float()
        return total, losses


def _item_values(output, gt_image, items, ray_depth_mask):
    passes, where = _color_passes(output, gt_image, items, ray_depth_mask)
    return {name: passes[p][kind] for name, (p, kind) in where.items()}


@torch.no_grad()
def frame_metrics(output, gt_image, items, ray_depth_mask=None):
    """The test-time colour metrics of run/train_ft.py:361-365 for a rendered
    frame (opt.test_color_loss_items): {"loss_<name>", "psnr_<name>"} device
    tensors from the same forward kernel as the training objective."""
    vals = _item_values(output, gt_image, list(items), ray_depth_mask)
    res = {}
    for name, v in vals.items():
        res["loss_" + name] = v
        res["psnr_" + name] = mse2psnr(v)
    return res
