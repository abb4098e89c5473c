"""Host layer of the training render: one render_rays_train call as stages -- query, size,
aggregate, head, composite, aux -- that never wait for the GPU unless the memory budget forces the one
count read; and the lazily computed dict the call leaves as last_train_aux."""
from __future__ import annotations

import torch

from . import _lib as L
from .aggregator import require_default_dims
from .render_eval import bg_channels
from .train import (AggregateFn, AggSpec, CompositeFn, CompositeSpec, PointTables, TRAIN_PRECISIONS, UsedPoints,
                    agg_params, used_points_device)

# device bytes a training batch reserves per sample slot: the forward's kept activations
# (train.Saved: 8 pairs x (h1..h4, PE_5, extras, masks, weights) + the sample's colour
# rows) and the backward's dz1..dz4 rows (train._Backward.pairs_chain)
TRAIN_BYTES_PER_SAMPLE = 8 * (4 * 1024 + 256 + 128 + 128 + 16) + 2660 + 8 * (4 * 1024 + 4) + 1024


class _TrainAux(dict):
    """render_rays_train's last_train_aux: keys whose values need the batch's
    host counts are computed when first read (so that the forward itself never
    waits for the GPU); ``"k" in aux`` is true for them without computing."""

    def __init__(self):
        super().__init__()
        self._lazy = {}

    def lazy(self, keys, fn):
        for k in keys:
            self._lazy[k] = fn

    def __contains__(self, k):
        return dict.__contains__(self, k) or k in self._lazy

    def __missing__(self, k):
        fn = self._lazy.get(k)
        if fn is None:
            raise KeyError(k)
        vals = fn()
        for kk in list(self._lazy):
            if self._lazy[kk] is fn:
                del self._lazy[kk]
        self.update(vals)
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if k in self else default


def train_budget(model, dev) -> int:
    """Bytes of per-sample training buffers a sync-free forward may reserve:
    train_memory_budget, or (None) a quarter of the device's memory."""
    if model.train_memory_budget is not None:
        return int(model.train_memory_budget)
    if model._budget_dev is None:
        model._budget_dev = torch.cuda.get_device_properties(dev).total_memory // 4
    return model._budget_dev


def march_aux(model, rays, qp, bufs, R, Rv, xyz, opacity):
    """weight [1,R'',SR,K] (detached: the aggregator's normalised weight),
    blend_weight [1,R'',SR,1] (detached), conf_coefficient [1,R'',SR,K]
    (gradiant_clamp of the gathered conf: straight-through gradient to
    points_conf, point_aggregators.py:724-726, 810-813; empty slots gather
    point 0 as torch.clamp(pidx, 0) does; 1 without a conf table) and
    sample_pidx, in pnr_query_compact's row order -- the reference's
    [1, R'', SR, ...] tensors of the same rays."""
    opt, np_ = model.opt, model.neural_points
    SR, K = opt.SR, opt.K
    dev = opacity.device
    f32 = dict(dtype=torch.float32, device=dev)
    pidx = torch.empty((1, Rv, SR, K), dtype=torch.int32, device=dev)
    scratch3 = [torch.empty((1, Rv, SR, 3), **f32) for _ in range(3)]
    rmask = torch.empty((1, R), dtype=torch.int8, device=dev)
    L.check(L.lib().pnr_query_compact(L.ctypes.byref(rays), L.ctypes.byref(qp), L.ctypes.byref(bufs.c), Rv,
                                      L.ptr(pidx), L.ptr(scratch3[0]), L.ptr(scratch3[1]),
                                      L.ptr(scratch3[2]), L.ptr(rmask), L.stream_ptr(dev)),
            "pnr_query_compact")
    weight = torch.empty((1, Rv, SR, K), **f32)
    blend = torch.empty((1, Rv, SR, 1), **f32)
    op = opacity.detach().contiguous()
    L.check(L.lib().pnr_march_aux(L.ctypes.byref(rays), L.ctypes.byref(qp), L.ctypes.byref(bufs.c),
                                  L.ptr(xyz), L.ptr(op), Rv, L.ptr(weight), L.ptr(blend), L.stream_ptr(dev)),
            "pnr_march_aux")
    aux = {"weight": weight, "blend_weight": blend, "sample_pidx": pidx, "conf_coefficient": 1}
    if np_.points_conf is not None:
        cf = np_.points_conf.reshape(-1)[pidx.clamp(min=0).long()]
        aux["conf_coefficient"] = cf - (cf - torch.clamp(cf, 1e-4, 1.0)).detach()
    return aux


class _TrainCall:
    """One render_rays_train call on model (a NeuralPointsRayMarching)."""

    def __init__(self, model, campos, camrot, raydir, near, far, bg_color):
        self.m, self.np_, self.opt = model, model.neural_points, model.opt
        require_default_dims(self.opt, "render_rays_train")   # before any launch: the training kernels are 32-wide, order 2
        if self.np_.points_embeding.dtype != torch.float32:
            raise L.PnrError("training needs an fp32 points_embeding (NeuralPoints(emb_dtype=torch.float32))")
        model._sync_rw2c()
        L.require_gpu(raydir)
        self.dev, self.R = raydir.device, raydir.shape[0]
        self.C = model.aggregator.C
        self.bg = bg_channels(bg_color, self.C, self.dev)
        self.campos = campos.reshape(3).float().contiguous()
        self.camrot = camrot.reshape(3, 3).float().contiguous()
        self.rd = raydir.float().contiguous()
        self.near, self.far = near, far
        self.xyz = self.np_.xyz.detach().contiguous()

    def run(self):
        self.query()
        self.size()
        feat = self.head(self.aggregate())
        out = self.composite(feat)
        self.aux(out)
        return out

    def query(self):
        """The query, and the list of the points this batch references (block1.0's point half is
        computed for them only).  No host read: the kernels take the device counts (samples:
        counts[1], used points: counts[5]) with capacity-sized buffers, and the counts travel to
        pinned memory behind an event that the backward (or last_counts) waits on -- the forward
        never drains the GPU."""
        self.bufs, self.hp, self.rays, self.qp = self.np_.querier.run(self.xyz, self.rd, self.campos, self.camrot,
                                                                      self.near, self.far, bufs=None)
        rows, row_map = used_points_device(self.bufs, self.opt.K, self.xyz.shape[0])
        self.used = UsedPoints(rows, row_map, self.bufs.counts[5:6])
        self.counts = self.m.last_counts = self.bufs.read_counts_async()

    def size(self):
        """The sample capacity that sizes the saved activations (train.Saved) and the backward's dz
        rows: every slot of the batch (R * SR, no host read) while that fits the memory budget, else
        this batch's valid-sample count (the one host read, counted in train_count_reads)."""
        self.S_cap = self.R * self.opt.SR
        if self.S_cap * TRAIN_BYTES_PER_SAMPLE > train_budget(self.m, self.dev):
            self.S_cap = max(int(self.bufs.read_counts()["S_valid"]), 1)
            self.m.train_count_reads += 1

    def aggregate(self):
        m, np_ = self.m, self.np_
        n = self.xyz.shape[0]

        def tab(t, c):
            return None if t is None else t.reshape(n, c)

        if m.train_precision not in TRAIN_PRECISIONS:
            raise L.PnrError(f"train_precision {m.train_precision!r}: 'fp32h2', 'fp32x3' or 'fp32'")
        self.spec = spec = AggSpec(
            m.aggregator, self.bufs.samples(self.rd, self.S_cap), self.S_cap,
            PointTables(self.xyz, campos=self.campos, camrot=self.camrot, rw2c=np_.rw2c_table()),
            used=self.used, precision=m.train_precision, counts=self.counts, keep=(self.bufs, self.rd),
            keep_saved=m.keep_train_saved)
        feat = AggregateFn.apply(spec, np_.points_embeding.reshape(n, 32), tab(np_.points_color, 3),
                                 tab(np_.points_dir, 3), tab(np_.points_conf, 1),
                                 np_.xyz if np_.xyz.requires_grad else None, *agg_params(m.aggregator))
        if spec.h2_fallback:
            m.h2_fallbacks += 1
        return feat

    def head(self, feat):
        """The upstream colour head (C_out = 3): [alpha, rgb] rows."""
        if self.C != 3:
            return feat
        return self.m.aggregator.apply_rgb_head(feat, n_dev=self.bufs.counts[1:2], n=self.S_cap)

    def composite(self, feat):
        opt = self.opt
        cp = L.CompositeParams(float(opt.vsize[2]), int(opt.raydist_mode_unit), self.C, None)
        cspec = CompositeSpec(self.rays, self.qp, self.bufs, cp, self.R, opt.SR, self.C,
                              keep=(self.campos, self.camrot, self.rd, self.hp), counts=self.counts)
        # bg: differentiable (the fork optimises bg_color, mvs_points_volumetric_model.py:92-94)
        return CompositeFn.apply(cspec, feat, self.bg)

    def aux(self, out):
        """What the call leaves on the model: the query buffers for the conf losses, and last_train_aux,
        whose groups are computed when first read (they need host counts)."""
        m, counts, dev = self.m, self.counts, self.dev
        rows = self.used.rows
        m._train_conf_src = self.bufs
        aux = _TrainAux()

        # rows of the point table this batch can give a gradient: the referenced points, and point 0
        # (empty slots gather it in conf_coefficient) -- parallel.GradReducer reduces only these across
        # ranks (unique: pnr_used_points lists each referenced point once, ascending; the appended
        # point 0 is dropped (-1) when it is already referenced)
        def touched():
            nu = counts.get()["n_used"]
            u = rows[:nu].long()
            zero = torch.zeros(1, dtype=torch.long, device=dev)
            if nu:
                zero = torch.where(u[:1] == 0, zero - 1, zero)
            return {"touched_rows": torch.cat([u, zero]), "touched_count": nu + 1}

        aux.lazy(("touched_rows", "touched_count"), touched)
        if m.keep_train_saved:
            aux["saved"] = self.spec.saved
        if self.np_.points_conf is not None or m.wants_aux():
            rays, qp, bufs, R, xyz, op = self.rays, self.qp, self.bufs, self.R, self.xyz, out[1]
            aux.lazy(("weight", "blend_weight", "sample_pidx", "conf_coefficient"),
                     lambda: march_aux(m, rays, qp, bufs, R, counts.get()["R_valid"], xyz, op))
        m.last_train_aux = aux
