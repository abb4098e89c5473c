"""The render module (the north-star hot path; its host layer: DESIGN.md 30).

``NeuralPointsRayMarching`` mirrors
models/neural_points_volumetric_model.py:230-389 (forward(**input) -> dict with
coarse_raycolor / coarse_point_opacity / coarse_is_background / coarse_mask /
queried_shading / ray_mask) over a ``NeuralPoints`` cloud (neural_points.py,
re-exported here), whose opt.wcoord_query picks the querier.

World grid (wcoord_query > 0, querier.py): the fused MI355X path
    pnr_query  (grid-resident march + layered KNN, device-side compaction)
 -> pnr_aggregate_fwd (gather + weights + PE + MFMA MLP + K-sum + colour MLP)
 -> pnr_composite_fwd (ray_dist + alpha composite + fill_invalid)
with one small device->host read of the sample counts per ray batch (to size
the feature buffer) and no ``raypos[R,400,3]`` / ``[R,SR,K,38]`` intermediates
(render_rays, render_rays_train; render_eval.py, render_train.py).

Perspective frustum (wcoord_query 0, querier_p.py): the reference's forward as
its seams (NeuralPoints.forward on pnr_pquery -> PointAggregator.forward ->
ray_march.py), differentiable; or, for an evaluation frame, the same fused chain
on pnr_pquery_build / pnr_pquery_bufs -> aggregate -> pnr_composite_fwd_p
(render_pixels).

``forward`` is inputs -> route -> frame -> assemble: one record of the call's
inputs made scalar once (ForwardInputs), one place that picks among "train",
"eval", "seams" and "pixels" (route), one record every route returns (Frame) and
one function that makes the output dict of it (assemble).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import torch
import torch.nn as nn

from . import _lib as L
from .aggregator import PointAggregator, require_default_dims
from .losses import _SparseConfLoss, _ZeroOneConfLoss
from .neural_points import NeuralPoints
from .querier import camera_tables
from .querier_p import check_supported
from .ray_march import fill_invalid, march_hit_rays, perspective_ray_dist
from .render_eval import (EAGER, QUEUED, PixelBatch, RayBatch, RenderGraph, _CallQueue, _PixelCall,  # noqa: F401
                          _RenderCall, _RenderState, bg_channels, query_params, with_h2_fallback)
from .render_train import TRAIN_BYTES_PER_SAMPLE, _TrainAux, _TrainCall, march_aux  # noqa: F401


# The default is fp32h2, the measured headline path (fp32-accurate: the same
# render tolerance as fp32, tests/test_gpu_x3.py; an activation beyond f16's range
# re-renders the call on fp32x3).
# fp32: the reference's arithmetic on v_mfma_f32_32x32x2_f32.  fp32x3: the same
# fp32 GEMMs as exact 3-way bf16 splits on v_mfma_f32_32x32x16_bf16 (six cross
# products, fp32-accurate; pnr_aggregate_fwd_x3).  fp32h2: the same GEMMs as 2-way
# f16 splits on v_mfma_f32_32x32x16_f16 (three products, fp32-accurate;
# pnr_aggregate_fwd_h2).  bf16: bf16 operands (config c5).
PRECISIONS = ("fp32", "fp32x3", "fp32h2", "bf16")

# forward's extra outputs with opt.prob == 1, in pnr_probe's argument order
PROBE_KEYS = ("ray_max_shading_opacity", "ray_max_sample_loc_w", "ray_max_far_dist", "shading_avg_color",
              "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding")


# the output dict of forward: key -> the Frame field it is a [1,R,...] view of
FRAME_KEYS = (("coarse_raycolor", "color", (-1,)), ("coarse_point_opacity", "opacity", (-1,)),
              ("coarse_is_background", "is_bg", (1,)), ("ray_mask", "ray_mask", ()))
# neural_points_volumetric_model.py:335-338
AUX_KEYS = ("weight", "blend_weight", "conf_coefficient")


@dataclass
class ForwardInputs:
    """One forward's inputs, every host number read once (the only .item() of near / far / h / w)."""
    campos: Any
    camrotc2w: Any
    raydir: Any        # [R,3]
    pixel_idx: Any
    near: float
    far: float
    h: Any             # int, or None where nothing reads it (a world model without the 2-D renderer)
    w: Any
    intrinsic: Any
    bg_color: Any      # None when bg_ray is passed
    gt_image: Any
    focal: Any = None


@dataclass
class Frame:
    """What every route of forward returns: render_rays' four outputs ([R,..] or [1,R,..]), ray_valid
    ([R]: queried_shading is one minus it), and the optional aux (AUX_KEYS) and probe (PROBE_KEYS) dicts."""
    color: Any
    opacity: Any
    is_bg: Any
    ray_mask: Any
    ray_valid: Any
    aux: Any = None
    probe: Any = None


class NeuralPointsRayMarching(nn.Module):
    """neural_points_volumetric_model.NeuralPointsRayMarching, fused HIP path."""

    def __init__(self, opt, neural_points: NeuralPoints, aggregator: PointAggregator | None = None,
                 chunk_rays: int | None = None, precision: str = "fp32h2", fused_perspective: bool = False):
        """fused_perspective: forward() of a perspective model (wcoord_query 0) renders an evaluation
        call that wants no aux outputs through render_pixels instead of the reference-shaped seams."""
        super().__init__()
        if precision not in PRECISIONS:
            raise L.PnrError(f"precision {precision!r}: one of {PRECISIONS}")
        self.precision = precision
        self.fused_perspective = bool(fused_perspective)
        # render_rays_train: "fp32h2" (forward chain and the weight / point-half gradient GEMMs on
        # f16-split MFMA, fp32-accurate: the measured default), "fp32x3" (split-bf16 MFMA,
        # fp32-accurate) or "fp32" (native fp32 MFMA)
        self.train_precision = "fp32h2"
        self.p1_side_stream = True        # fp32h2 sync-free calls: P1 beside the query (render_eval: start_p1_side)
        self.p1_used_only = True          # bf16: P1 for the referenced points only (render_eval: aggregate_chunk)
        # bf16: the aggregated features themselves in bf16 (pnr_aggregate_fwd_bf16_hf ->
        # pnr_composite_fwd_hf: half the feature bytes written and read)
        self.bf16_features = True
        self.p1_side_max_points_per_ray = 4.0
        self.keep_train_saved = False   # tests: last_train_aux["saved"] = the forward's kept activations
        # render_rays_train sizes its per-sample buffers for every slot of the batch while
        # R * SR * TRAIN_BYTES_PER_SAMPLE fits this many bytes (None: a quarter of the
        # device memory), else it reads the batch's valid-sample count (train_count_reads)
        self.train_memory_budget = None
        self.train_count_reads = 0
        self._h2_blocked_key = None   # weights whose activations left the f16 range (render_rays)
        self.h2_fallbacks = 0
        self.opt = opt
        self.neural_points = neural_points
        self.aggregator = aggregator if aggregator is not None else PointAggregator(opt).to(neural_points.device)
        self.chunk_rays = chunk_rays
        self._state = _RenderState()     # query buffers + aggregate scratch of the eager path
        self._queue = _CallQueue()       # render_rays(sync=False) calls awaiting finish(), and their sizing estimate
        self.overflow_rerenders = 0
        # fork's 2-D CNN after the composite (neural_points_volumetric_model.py:258-260, 343-344)
        self.neural_render_2d = None
        if getattr(opt, "neural_render", "none") == "cnn":
            from .neural_render import NeuralRenderer
            self.neural_render_2d = NeuralRenderer(input_dim=128).to(neural_points.device)
        self._last_counts = None
        self._train_conf_src = None   # query buffers of the last render_rays_train (zero_one_conf_loss)
        self.last_train_aux = None    # _TrainAux of the last render_rays_train
        self._budget_dev = None       # a quarter of the device's memory, once asked for (render_train.train_budget)
        self._rw2c_key = None
        self.path = self.path_why = None   # the route of the last forward and its reason (route)
        if getattr(opt, "which_render_func", "radiance") != "radiance" or \
                getattr(opt, "which_blend_func", "alpha") != "alpha" or \
                getattr(opt, "which_tonemap_func", "off") != "off":
            raise L.PnrError("libpnr implements radiance render, alpha blend and tone map 'off'")

    def _world_only(self, who: str):
        if self.neural_points.perspective:
            raise L.PnrError(f"{who}: the fused frame is world-query only; with wcoord_query 0 call render_pixels "
                             "(an evaluation frame) or the module (forward)")

    def _sync_rw2c(self):
        """The aggregator renders with NeuralPoints.Rw2c (neural_points.py:289;
        applied to view dirs, distances and point dirs at
        point_aggregators.py:506, 526, 566): copied into the aggregator's
        buffer whenever the points' Rw2c tensor (storage or version) changes."""
        rw = self.neural_points.Rw2c
        key = (rw.data_ptr(), rw._version, tuple(rw.shape))
        if key != self._rw2c_key:
            # per-point [N,3,3]: the kernels read it from pnr_points.rw2c
            # (NeuralPoints.tables), the uniform matrix stays the identity
            self.aggregator.set_rw2c(rw.detach() if rw.dim() == 2 else None)
            self._rw2c_key = key

    @torch.no_grad()
    def render_rays(self, campos, camrot, raydir, near, far, bg_color, force_grid=False, events=None,
                    reuse_p1=False, sync=True, ray_cam=None, query_stream=None):
        """Fused query -> aggregate -> composite for one ray batch [R,3].
        Returns ray_color [R,C], opacity [R,SR], is_bg [R], ray_mask [R] (int8).
        ``events``: optional list that receives (stage, start, end) HIP events
        recorded on the launch stream around each stage.
        block1.0's per-point half (P1, which does not depend on the camera)
        is prepared model state like the weight packs and the grid (DESIGN
        §36): built by the first call into a table the render state keeps,
        and again only after points_embeding or block1.0 changed (new storage
        or an in-place change, which bumps ``_version``), the point count or
        the precision.  ``reuse_p1`` is kept for its callers and changes
        nothing (with ``PNR_P1_PER_FRAME=1`` in the environment every call
        builds P1 again unless it is passed: the behaviour before, for A/B).
        A write that changes neither storage nor version (through ``.data``,
        by a raw-pointer kernel) is not seen, exactly as for the grid below:
        pass ``force_grid=True`` after it, which drops the grid and P1.
        ``ray_cam`` (int32 [R], optional): camera index of each ray into
        campos [n_cams,3] / camrot [n_cams,3,3] -- several frames' rays
        rendered as one batch (``render_views``).

        ``sync=False``: no host synchronisation at all.  The decoded-feature
        buffer is sized from the largest valid-sample count per ray seen so far
        (x 1.25) instead of this batch's count, and the two checks a
        synchronous call makes -- the count fits, the fp32h2 activations stayed
        in range -- are deferred to ``finish()``, which re-renders a call that
        failed either of them into the same output tensors.  The outputs are
        valid once ``finish()`` returned.  The first call (no estimate yet)
        runs synchronously.

        ``query_stream`` (sync-free calls): run the call's query on this HIP
        stream instead of the launch stream, so it overlaps the previous call's
        aggregate (the query is memory-latency bound, the aggregate MFMA bound,
        and one query workgroup fits beside a k_pairs_h2 workgroup on a CU).  The
        aggregate waits for it; the query waits only for the launch-stream work
        that last read its buffers (two sets, alternating) and, when the points
        changed since the last such call (new storage or version, or
        ``force_grid``), for the whole launch stream.  The call's own copies of
        its inputs (contiguous rays, camera tables) are made on the query
        stream; the caller makes ``raydir`` / ``campos`` / ``camrot`` /
        ``ray_cam`` themselves ready on that stream.  A write to the points
        that changes neither their storage nor their version (through ``.data``,
        by a raw-pointer kernel) is not seen: pass ``force_grid=True`` after it.

        fp32h2: the f16 split holds activations below 65504 only.  Each call
        reads the launches' range flag once (a 4-byte read after the last
        chunk); if an activation left the f16 range, the call is rendered again
        on the fp32x3 path (bf16 split: same accuracy, fp32 range) and h2 stays
        off for these weights until they change (``h2_fallbacks`` counts it)."""
        self._sync_rw2c()
        q = self._queue
        if sync or q.sv_per_ray is None:
            q.flush(self)   # a synchronous call reads (and may clear) the shared range flag and the counts
        batch = RayBatch(campos, camrot, raydir, near, far, bg_color, ray_cam)
        prec = self._precision_now()
        opts = dict(force_grid=force_grid, events=events)
        if not sync and q.sv_per_ray is not None:
            out, rec = self._render_rays(QUEUED, prec, batch, self._state, reuse_p1=reuse_p1, query_stream=query_stream,
                                         capacity=q.sv_per_ray * 1.25, **opts)
            q.pending.append(rec)
            return out
        return with_h2_fallback(self, prec, events, lambda p, first: self._render_rays(
            EAGER, p, batch, self._state, reuse_p1=reuse_p1 and first, **opts)[0])

    @torch.no_grad()
    def render_pixels(self, campos, camrotc2w, pixel_idx, h, w, intrinsic, near, far, bg_color, events=None,
                      reuse_p1=False, frame=False):
        """The fused evaluation frame of a perspective model (wcoord_query 0): pnr_pquery_build
        once, then per chunk of chunk_rays pixels pnr_pquery_bufs -> the precision's aggregate over the valid
        samples -> pnr_composite_fwd_p.  No gathered pair tensor, one host read (the counts) per chunk.
        pixel_idx: [R,2] (x, y), or None for the whole h x w frame in row-major order.  Returns render_rays'
        (ray_color [R,C], opacity [R,SR], is_bg [R], ray_mask [R] int8) and sets last_counts; ray_mask is the
        querier's (a hit ray without any neighbour keeps 1 and composites to the background).  One camera per
        call.  It never applies shpnt_jitter (the sample depths are the voxel centres).  events, reuse_p1 and
        the fp32h2 fallback to fp32x3 as in render_rays; events also receives the ("build", ...) stage.
        frame=True (forward's fused route): the same as a Frame, whose ray_valid ([R] bool: the ray has a
        valid sample) forward's queried_shading needs."""
        opt = self.opt
        if not self.neural_points.perspective:
            raise L.PnrError("render_pixels renders the perspective query (wcoord_query 0); this model queries the "
                             "world grid: call render_rays")
        if self.precision == "bf16":
            raise L.PnrError("render_pixels: precision 'bf16' is not supported (fp32, fp32x3 or fp32h2)")
        if int(opt.K) > 8:
            raise L.PnrError(f"render_pixels: K = {int(opt.K)} neighbours per sample; the fused aggregate takes "
                             "1 .. 8")
        check_supported(opt)
        self._queue.flush(self)
        self._sync_rw2c()
        batch = PixelBatch.of(self.neural_points.xyz.device, campos, camrotc2w, pixel_idx, h, w, intrinsic, near, far,
                              bg_color)
        out = with_h2_fallback(self, self._precision_now(), events, lambda p, first: _PixelCall(
            self, p, batch, self._state, events=events, reuse_p1=reuse_p1 and first).run()[0])
        return Frame(*out) if frame else out[:4]

    def _render_rays(self, mode, precision, batch, state, **options):
        """One render call (render_eval._RenderCall and its modes) -> (outputs, its _PendingCall or None)."""
        self._world_only("render_rays / RenderGraph")   # the one door of every fused world render
        if precision == "bf16":
            require_default_dims(self.opt, "precision 'bf16'")
        return _RenderCall(self, mode, precision, batch, state, **options).run()

    def render_camera(self, campos, camrotc2w, intrinsic, H, W, near, far, bg_color, dir_norm=False, **kw):
        """Render one camera's H x W frame: ``rays.camera_rays`` (pnr_camera_rays:
        the directions made on the device, no table uploaded) followed by
        ``render_rays`` with its keyword arguments.  intrinsic: [3,3] or a focal
        length with the principal point at the frame's centre."""
        from .rays import camera_rays
        raydir = camera_rays(intrinsic, camrotc2w, H, W, dir_norm=dir_norm, device=self.neural_points.xyz.device)
        return self.render_rays(campos, camrotc2w, raydir, near, far, bg_color, **kw)

    def render_views(self, views, near, far, bg_color, force_grid=False, events=None, reuse_p1=False, sync=True):
        """Render several frames' ray batches -- views = [(campos [3], camrot
        [3,3], raydir [R_i,3]), ...], e.g. the N band shares one rank renders
        per multi-GPU step -- as ONE batch: one query, one aggregate and one
        composite launch over all of them (pnr_rays.ray_cam), so no per-call
        cost grows with the number of views.  Returns one (ray_color, opacity,
        is_bg, ray_mask) tuple per view (views of the batch outputs); last_counts
        / finish() report the batch."""
        dev = views[0][2].device
        campos = torch.stack([v[0].reshape(3).float() for v in views]).to(dev)
        camrot = torch.stack([v[1].reshape(3, 3).float() for v in views]).to(dev)
        sizes = [int(v[2].shape[0]) for v in views]
        raydir = torch.cat([v[2].reshape(-1, 3).float() for v in views]).contiguous()
        ray_cam = torch.repeat_interleave(torch.arange(len(views), dtype=torch.int32, device=dev),
                                          torch.tensor(sizes, device=dev), output_size=sum(sizes))
        out = self.render_rays(campos, camrot, raydir, near, far, bg_color, force_grid, events, reuse_p1, sync,
                               ray_cam=ray_cam)
        return [tuple(t.split(sizes)[i] for t in out) for i in range(len(views))]

    def _precision_now(self):
        prec = self.precision
        if prec == "fp32h2" and self._h2_blocked_key is not None:
            if self._h2_blocked_key == self.aggregator.h2_key():
                prec = "fp32x3"
            else:
                self._h2_blocked_key = None
        return prec

    def _block_h2(self):
        self.aggregator.h2_reset_range()
        self._h2_blocked_key = self.aggregator.h2_key()
        self.h2_fallbacks += 1

    @torch.no_grad()
    def finish(self, upto=None):
        """Complete every ``render_rays(sync=False)`` call issued since the last
        finish() -- or only the oldest ``upto`` of them, so the caller can keep
        the next calls queued on the GPU while the host checks these: one host
        synchronisation (on the last completed call), then the deferred checks.
        A call whose valid samples overflowed its feature buffer, or (fp32h2) any
        call when an activation left the f16 range, is rendered again
        synchronously into its own output tensors (a raised range flag is shared
        by the calls still in flight, so then every pending call is completed and
        the later ones' counts are kept for the next finish()).  Returns the
        per-call sample counts (the ``last_counts`` dict of each call, in issue
        order)."""
        return self._queue.finish(self, upto)

    # the queue's state under the names it had on the module
    _pending = property(lambda self: self._queue.pending)
    _sv_per_ray = property(lambda self: self._queue.sv_per_ray,
                           lambda self, v: setattr(self._queue, "sv_per_ray", v))

    @property
    def last_counts(self):
        """Sample counts of the last render call (dict); a training call leaves a
        pending CountsHandle that is read here, when first asked for."""
        c = self._last_counts
        if c is not None and not isinstance(c, dict):
            c = self._last_counts = c.get()
        return c

    @last_counts.setter
    def last_counts(self, v):
        self._last_counts = v

    def render_rays_train(self, campos, camrot, raydir, near, far, bg_color):
        """Differentiable render of one training ray batch [R,3] (SURVEY 8(a)
        a17): same query / aggregate / composite as render_rays, with autograd
        through pnr_aggregate_fwd_train -> pnr_aggregate_bwd_pairs and
        pnr_composite_fwd -> pnr_composite_bwd (train.py; the call's stages:
        render_train._TrainCall).  Returns ray_color
        [R,C] (requires grad w.r.t. points_embeding / color / dir / conf and the
        aggregator parameters), opacity [R,SR], is_bg [R], ray_mask [R]."""
        require_default_dims(self.opt, "render_rays_train")
        self._world_only("render_rays_train")
        return _TrainCall(self, campos, camrot, raydir, near, far, bg_color).run()

    def wants_aux(self) -> bool:
        """The reference aggregator returns weight / conf_coefficient (and the
        module puts them with blend_weight into its output,
        neural_points_volumetric_model.py:335-338) unless no loss reads them
        (point_aggregators.py:814-815)."""
        o = self.opt
        return (getattr(o, "sparse_loss_weight", 0) > 0 or "conf_coefficient" in getattr(o, "zero_one_loss_items", ())
                or getattr(o, "prob", 0) != 0)

    @torch.no_grad()
    def eval_aux(self, campos, camrot, raydir, near, far, opacity):
        """forward()'s weight / blend_weight / conf_coefficient for an
        evaluation render (render_rays keeps no per-pair state): the batch's
        query again, then pnr_query_compact + pnr_march_aux on the rendered
        opacity.  conf_coefficient carries no graph here (no_grad render)."""
        self._world_only("eval_aux")
        np_ = self.neural_points
        cp, cr = camera_tables(campos, camrot, None)
        xyz = np_.xyz.detach().contiguous()
        bufs, _hp, rays, qp = np_.querier.run(xyz, raydir.float().contiguous(), cp, cr, near, far, bufs=None)
        return march_aux(self, rays, qp, bufs, raydir.shape[0], bufs.read_counts()["R_valid"], xyz, opacity)

    @torch.no_grad()
    def probe_maps(self, campos, camrot, raydir, near, far, opacity):
        """The seven opt.prob == 1 outputs of the reference's forward
        (neural_points_volumetric_model_ori.py:351-372; PROBE_KEYS) for an
        evaluation render, in full ray order: the batch's query again (like
        eval_aux, chunk_rays at a time), then one pnr_probe launch per chunk on
        the rendered opacity [R,SR] -- no compaction, no [R'',SR,K,*] tensors, no
        host read.  Shapes [1,R,1] / [1,R,3] / [1,R,32]; None for an absent
        point table; rows of rays without a neighbour are zeros."""
        require_default_dims(self.opt, "probe_maps (opt.prob == 1, the point-growing probe)")
        self._world_only("probe_maps")
        np_ = self.neural_points
        raydir = raydir.reshape(-1, 3).float().contiguous()
        dev = raydir.device
        R, SR = raydir.shape[0], self.opt.SR
        cp, cr = camera_tables(campos, camrot, None)
        xyz = np_.xyz.detach().contiguous()
        pts, _keep = np_.tables(cp, cr, bf16=True)
        op = opacity.detach().reshape(R, SR).float().contiguous()

        def buf(c, have=True):
            return torch.empty((1, R, c), dtype=torch.float32, device=dev) if have else None

        out = dict(ray_max_shading_opacity=buf(1), ray_max_sample_loc_w=buf(3), ray_max_far_dist=buf(1),
                   shading_avg_color=buf(3, np_.points_color is not None),
                   shading_avg_dir=buf(3, np_.points_dir is not None),
                   shading_avg_conf=buf(1, np_.points_conf is not None), shading_avg_embedding=buf(32))
        chunk = max(1, self.chunk_rays or R)
        bufs = None
        for c0 in range(0, R, chunk):
            c1 = min(c0 + chunk, R)
            bufs, _hp, rays, qp = np_.querier.run(xyz, raydir[c0:c1], cp, cr, near, far, bufs=bufs)
            L.check(L.lib().pnr_probe(L.ctypes.byref(rays), L.ctypes.byref(qp), L.ctypes.byref(bufs.c),
                                      L.ctypes.byref(pts), L.ptr(op[c0:c1]),
                                      *(L.ptr(None if out[k] is None else out[k][0, c0:c1]) for k in PROBE_KEYS),
                                      L.stream_ptr(dev)), "pnr_probe")
        return out

    def probe_rays(self, campos, camrot, raydir, near, far, bg_color):
        """render_rays plus probe_maps for a ray batch [R,3] of any size
        (chunk_rays at a time), for callers that do not go through forward:
        dict of coarse_raycolor [1,R,C], coarse_point_opacity [1,R,SR],
        coarse_is_background [1,R,1], ray_mask [1,R] and the PROBE_KEYS maps."""
        raydir = raydir.reshape(-1, 3)
        color, opacity, is_bg, ray_mask = self.render_rays(campos, camrot, raydir, near, far, bg_color)
        return self.assemble(Frame(color, opacity, is_bg, ray_mask, ray_mask,
                                   probe=self.probe_maps(campos, camrot, raydir, near, far, opacity)))

    def _last_train(self, who: str):
        """(query buffers, their pnr_query_params) of the last training render, for the conf losses."""
        bufs = self._train_conf_src
        if bufs is None:
            raise L.PnrError(f"{who}: no training render yet (call render_rays_train / forward in "
                             "training mode first)")
        return bufs, query_params(bufs.SR, bufs.K)

    def zero_one_conf_loss(self, zero_epsilon: float = 1e-3):
        """zero_one_loss(conf_coefficient) of the last render_rays_train, computed
        per point: every entry of conf_coefficient is a function of one point's
        conf, so the mean over the [1, R'', SR, K] entries equals
        sum_p count_p f(conf_p) / entries (count_p = entries gathering point p,
        point 0 also collecting the empty slots) -- same value and gradient
        without the gather's scatter-add backward.  The counts come from the
        query's own neighbour lists on the device (the R'' rays' filled samples
        hold every non-negative entry of sample_pidx; the other
        R'' * SR * K - sum_p count_p entries are empty slots, gathered as point 0):
        no host read of R'' and no compaction (losses._ZeroOneConfLoss)."""
        bufs, qp = self._last_train("zero_one_conf_loss")
        conf = self.neural_points.points_conf.reshape(-1)
        return _ZeroOneConfLoss.apply(conf, bufs, qp.SR, qp.K, float(zero_epsilon))

    def sparse_conf_loss(self):
        """The sparse loss (base_rendering_model.py:652-662) of the last
        render_rays_train, sum(weight |1 - exp(-2 conf_coefficient)|) /
        (sum(weight) + 1e-6), computed per point like zero_one_conf_loss: with
        W_p the summed weight of the pairs that gather point p it equals
        sum_p W_p f(cc_p) / (sum_p W_p + 1e-6), and d conf_p = g W_p f'(cc_p) /
        (sum W + 1e-6) (gradiant_clamp's straight-through gradient).  The pair
        weights are recomputed from the query buffers as pnr_march_aux writes
        them (detached; empty slots weigh 0): no host read of R'', no
        compaction, no [1, R'', SR, K] tensors.  Without a conf table
        conf_coefficient is 1: a value without a gradient.  Bitwise repeatable
        (losses._SparseConfLoss)."""
        bufs, qp = self._last_train("sparse_conf_loss")
        np_ = self.neural_points
        return _SparseConfLoss.apply(np_.points_conf, np_.xyz.detach().contiguous(), bufs, qp)

    @staticmethod
    def zero_one_loss(val, zero_epsilon: float = 1e-3):
        """base_rendering_model.py:630-641: mean(log(v) + log(1 - v)), v clamped
        to [eps, 1 - eps]."""
        v = torch.clamp(val, zero_epsilon, 1 - zero_epsilon)
        return torch.mean(torch.log(v) + torch.log(1 - v))

    # ---------------------------------------------------------------- forward: inputs -> route -> frame -> assemble
    def _inputs(self, campos, raydir, gt_image, bg_color, camrotc2w, pixel_idx, near, far, focal, h, w, intrinsic):
        sized = self.neural_points.perspective or self.neural_render_2d is not None   # else nothing reads h, w

        def size(v):
            return L.host_scalar(v, int) if sized and v is not None else None

        near, far = L.host_scalar(near, float, torch.min), L.host_scalar(far, float, torch.max)
        return ForwardInputs(campos, camrotc2w, raydir.reshape(-1, 3), pixel_idx, near, far, size(h), size(w), intrinsic,
                             bg_color, gt_image, focal)

    def route(self, inputs: ForwardInputs):
        """(route, why) of a forward, kept as path / path_why:
        "train"  world model, a training step (model(...) then loss.backward(), as run/train_ft.py does: grad
                 mode, train() and a parameter or bg_color to train): render_rays_train
        "eval"   world model otherwise: render_rays (+ eval_aux, + probe_maps with opt.prob == 1)
        "pixels" perspective model with fused_perspective, when render_pixels computes the same: no training
                 step, no aux output wanted, no sample jitter to apply
        "seams"  perspective model otherwise: the reference's forward as its seams, differentiable."""
        opt = self.opt
        train = torch.is_grad_enabled() and self.training and (
            any(p.requires_grad for p in self.parameters())
            or (torch.is_tensor(inputs.bg_color) and inputs.bg_color.requires_grad))
        prob = getattr(opt, "prob", 0) == 1
        if train:
            require_default_dims(opt, "forward: a training step")
        if prob:
            require_default_dims(opt, "opt.prob == 1 (the point-growing probe)")
        if not self.neural_points.perspective:
            if train and prob:
                raise L.PnrError("opt.prob == 1 (the point-growing probe) is an evaluation render, as in the "
                                 "reference's probe_hole: call the module in eval() mode or under no_grad")
            r = ("train", "a training step") if train else ("eval", "no training step under way")
        else:
            if prob:
                raise L.PnrError("opt.prob == 1 (the point-growing probe) is world-query only")
            jitter = getattr(opt, "is_train", 0) != 0 and getattr(opt, "shpnt_jitter", "passfunc") != "passfunc"
            declined = [why for cond, why in ((not self.fused_perspective, "fused_perspective is off"),
                                              (train, "a training step"), (self.wants_aux(), "aux outputs wanted"),
                                              (jitter, "a sample jitter, which render_pixels never applies")) if cond]
            r = ("seams", declined[0]) if declined else ("pixels", "fused_perspective: an evaluation frame")
        self.path, self.path_why = r
        return r

    def _frame_train(self, i: ForwardInputs) -> Frame:
        color, opacity, is_bg, ray_mask = self.render_rays_train(i.campos, i.camrotc2w, i.raydir, i.near, i.far,
                                                                 i.bg_color)
        return Frame(color, opacity, is_bg, ray_mask, ray_mask, self.last_train_aux if self.wants_aux() else None)

    def _frame_eval(self, i: ForwardInputs) -> Frame:
        a = (i.campos, i.camrotc2w, i.raydir, i.near, i.far)
        color, opacity, is_bg, ray_mask = self.render_rays(*a, i.bg_color)
        aux = self.eval_aux(*a, opacity) if self.wants_aux() else None
        # neural_points_volumetric_model_ori.py:351-372
        probe = self.probe_maps(*a, opacity) if getattr(self.opt, "prob", 0) == 1 and color.shape[0] > 0 else None
        return Frame(color, opacity, is_bg, ray_mask, ray_mask, aux, probe)

    def _frame_pixels(self, i: ForwardInputs) -> Frame:
        for name in ("pixel_idx", "h", "w", "intrinsic"):
            if getattr(i, name) is None:
                raise L.PnrError(f"forward with wcoord_query 0 (the perspective query) needs {name}")
        return self.render_pixels(i.campos, i.camrotc2w, i.pixel_idx, i.h, i.w, i.intrinsic, i.near, i.far, i.bg_color,
                                  frame=True)

    def _frame_seams(self, i: ForwardInputs) -> Frame:
        """The reference's forward as its seams (neural_points_volumetric_model.py:288-341):
        NeuralPoints.forward's 14-tuple (pnr_pquery), PointAggregator.forward (the fused aggregate,
        differentiable), then ray_march.py's ray_dist, march and fill_invalid.  ray_mask is the querier's (the
        column's far id > 0): a hit ray without any neighbour keeps ray_mask 1 and composites to the background."""
        self._sync_rw2c()
        (s_color, s_rw2c, s_dir, s_conf, s_emb, s_pers, s_xyz, s_mask, s_loc, s_loc_w, s_dirs, ray_mask, vsize,
         grid_vox_sz) = self.neural_points({"pixel_idx": i.pixel_idx, "camrotc2w": i.camrotc2w, "campos": i.campos,
                                            "near": i.near, "far": i.far, "focal": i.focal, "h": i.h, "w": i.w,
                                            "intrinsic": i.intrinsic, "gt_image": i.gt_image, "raydir": i.raydir})
        feats, ray_valid, weight, conf = self.aggregator(s_color, s_rw2c, s_dir, s_conf, s_emb, s_pers, s_xyz, s_mask,
                                                         s_loc, s_loc_w, s_dirs, vsize, grid_vox_sz)
        # vsize[2]: the querier's (far - near) / z_depth_dim
        rd = perspective_ray_dist(s_loc[..., 2], ray_valid, float(vsize[2]), self.opt.raydist_mode_unit)
        color, opacity, blend_weight, bg_T = march_hit_rays(rd, ray_valid, feats, i.bg_color)
        color, opacity, is_bg, any_valid = fill_invalid(ray_mask, color, opacity, bg_T, ray_valid, i.bg_color)
        aux = None if weight is None else dict(weight=weight.detach(), blend_weight=blend_weight.detach(),
                                               conf_coefficient=conf)
        return Frame(color, opacity, is_bg, ray_mask, any_valid, aux)

    def assemble(self, frame: Frame, inputs: ForwardInputs | None = None) -> dict:
        """The output dict of a Frame: FRAME_KEYS, then coarse_mask, queried_shading, the aux and probe
        outputs and the 2-D renderer's final_coarse_raycolor.  Without inputs (probe_rays): FRAME_KEYS and
        the probe maps only."""
        R = frame.ray_mask.numel()
        out = {key: getattr(frame, field).view(1, R, *tail) for key, field, tail in FRAME_KEYS}
        if inputs is not None:
            out["coarse_mask"] = 1 - out["coarse_is_background"]
            out["queried_shading"] = (1 - frame.ray_valid.float().view(1, R, 1)).repeat(1, 1, 3)
            if frame.aux is not None:
                for k in AUX_KEYS:
                    out[k] = frame.aux[k]
        if frame.probe is not None:
            out.update(frame.probe)
        if inputs is not None and self.neural_render_2d is not None:
            out["final_coarse_raycolor"] = self.neural_render_2d(
                out["coarse_raycolor"].reshape(1, inputs.h, inputs.w, -1)).reshape(1, -1, 3)
        return out

    def forward(self, campos, raydir, gt_image=None, bg_color=None, camrotc2w=None, pixel_idx=None,
                near=None, far=None, focal=None, h=None, w=None, intrinsic=None, **kargs):
        """neural_points_volumetric_model.py:272-352 (+ fill_invalid :354-389);
        B = 1.  With opt.neural_render == "cnn" the fork's 2-D decoder
        (NeuralRenderer, :343-344) adds final_coarse_raycolor (needs h, w)."""
        if raydir.dim() == 3 and raydir.shape[0] != 1:
            raise L.PnrError("batch size B > 1 is not supported (the reference uses B = 1)")
        inputs = self._inputs(campos, raydir, gt_image, None if "bg_ray" in kargs else bg_color, camrotc2w, pixel_idx,
                              near, far, focal, h, w, intrinsic)
        name, _why = self.route(inputs)
        frame = {"train": self._frame_train, "eval": self._frame_eval, "pixels": self._frame_pixels,
                 "seams": self._frame_seams}[name](inputs)
        return self.assemble(frame, inputs)
