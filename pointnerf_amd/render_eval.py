"""Host layer of the evaluation render: a render_rays / finish() / RenderGraph call as stages over
the ray chunks, issuing kernels, events and stream waits in one fixed order; the typed records the calls leave;
the queue of sync=False calls and the fp32h2 fallback the module's entry points share."""
from __future__ import annotations

import gc
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import querier as Q
from . import querier_p as QP
from .train import used_points_buffers, used_points_device


def bg_channels(bg_color, C: int, dev):
    """bg_color as the composite reads it: fp32 [C] on dev, one value repeated
    C times; None stays None.  Differentiable (the fork optimises bg_color)."""
    if bg_color is None:
        return None
    bg = bg_color.to(dev).float().reshape(-1).contiguous()
    if bg.numel() not in (1, C):
        raise L.PnrError(f"bg_color must have 1 or {C} channels")
    return bg if bg.numel() == C else bg.expand(C).contiguous()


def query_params(SR, K) -> L.QueryParams:
    """The pnr_query_params of the kernels that only walk query buffers: their SR and K."""
    qp = L.QueryParams()
    qp.SR, qp.K = int(SR), int(K)
    return qp


# the inputs of one render call, as the caller gave them
RayBatch = namedtuple("RayBatch", "campos camrot raydir near far bg_color ray_cam", defaults=(None,))


class _Mode(NamedTuple):
    """What a caller of _render_rays may do."""
    side_p1: bool     # fp32h2: may run P1 on the side stream, beside the query
    used_only: bool   # bf16: may compute P1 for the referenced points only
    counts: str       # a chunk's counts: read "now" (they size it), copied to "pinned" or to "device" memory


EAGER = _Mode(False, True, "now")        # synchronous render_rays, finish()'s re-render, RenderGraph's sizing render
QUEUED = _Mode(True, True, "pinned")     # render_rays(sync=False), optionally with a query stream
WARMUP = _Mode(True, True, "device")     # RenderGraph's run before the capture (allocations, packs)
CAPTURE = _Mode(False, False, "device")  # RenderGraph's captured run: one stream, every point's P1 in the graph


@dataclass
class _PendingCall:
    """What a QUEUED call leaves for finish(), a CAPTURE call for RenderGraph.check()."""
    precision: str
    caps: list          # per chunk: (feature rows it was sized for, rays)
    counts: Any         # [n_chunks, 8] int32: pinned (QUEUED, valid behind event) or on the device
    range_flag: Any     # fp32h2: the packs' device range flag, else None
    range_host: Any     # QUEUED fp32h2: its pinned copy, taken after the call's launches
    event: Any          # QUEUED: recorded behind the call's last copy
    batch: RayBatch     # for finish()'s re-render ...
    force_grid: bool    # ... which forces the grid again when the call did
    out: tuple
    h2_key: tuple       # what a re-render must find unchanged: the weights ...
    grid_key: Any       # ... and the grid
    keep: tuple = ()    # CAPTURE: the packs the captured launches point into


def chunk_counts(rec: _PendingCall):
    """(feature rows the chunk was sized for, its rays, its counts dict) per chunk of a completed call."""
    for (cap, rays), h in zip(rec.caps, rec.counts.tolist()):
        yield cap, rays, Q.counts_dict(h, n_used=False)


class _CallQueue:
    """The render_rays(sync=False) calls of one module that await finish(), and what sizes the next one.
    It holds no reference to the module (the two would form a cycle and the module's device memory would
    wait for a cyclic collection): the module passes itself to flush / finish."""

    def __init__(self):
        self.pending = []        # _PendingCall records, in issue order
        self.done = []           # counts of calls a synchronous render completed, for the next finish()
        self.sv_per_ray = None   # largest valid samples per ray seen (feature-buffer sizing)

    def observe(self, counts, rays):
        r = counts["S_valid"] / max(rays, 1)
        self.sv_per_ray = r if self.sv_per_ray is None else max(self.sv_per_ray, r)

    def flush(self, m):
        """Before a call that reads (and may clear) the shared range flag and the counts: complete the pending
        calls so none of their checks is lost; their counts stay queued for the caller's next finish()."""
        if self.pending:
            self.done = self.finish(m) + self.done

    def finish(self, m, upto=None):
        """NeuralPointsRayMarching.finish of module m."""
        if upto is None:   # freeing a collected GridHandle synchronises the device: not while later calls stay queued
            Q.release_deferred()
        done = self.done
        n_all = len(done) + len(self.pending)
        k = n_all if upto is None else min(int(upto), n_all)
        need = k - len(done)
        if need > 0:
            head = self.pending[:need]
            head[-1].event.synchronize()
            # the range flags as copied to pinned memory behind each call's event (a
            # .item() here would queue behind -- and wait for -- the later calls)
            if need < len(self.pending) and any(int(r.range_host[0]) != 0 for r in head if r.range_flag is not None):
                head = self.pending
                head[-1].event.synchronize()
            self.pending = self.pending[len(head):]
            done = done + self.complete(m, head)
        self.done = done[k:]
        return done[:k]

    def complete(self, m, pend):
        """finish()'s checks on calls whose last kernels have completed."""
        # every fp32h2 call's own range flag (the packs, and their flag, are rebuilt when the weights change between
        # calls), read from the call's pinned copy taken after its launches: the raised ones, by storage
        h2 = [r for r in pend if r.range_flag is not None]
        raised = {r.range_flag.data_ptr(): r.range_flag for r in h2 if int(r.range_host[0]) != 0}
        if raised:
            cur = m.aggregator.h2_key()
            for f in raised.values():
                f.zero_()
            m.aggregator.h2_reset_range()
            if any(r.h2_key == cur for r in h2):
                m._h2_blocked_key = cur
            m.h2_fallbacks += 1
        counts = []
        for rec in pend:
            tot = dict(S_filled=0, S_valid=0, R_hit=0, R_valid=0, n_pairs=0, n_cand=0)
            over = False
            for cap, rays, c in chunk_counts(rec):
                self.observe(c, rays)
                over |= c["S_valid"] > cap
                for k in tot:
                    tot[k] += c[k]
            rec_bad = rec.range_flag is not None and rec.range_flag.data_ptr() in raised
            if over or rec_bad:
                if rec.h2_key != m.aggregator.h2_key() or rec.grid_key != m.neural_points.querier.grid.key:
                    raise L.PnrError("a render_rays(sync=False) call must be re-rendered, but the weights or the "
                                     "points changed before finish(): call finish() before modifying the model")
                out, _ = m._render_rays(EAGER, "fp32x3" if rec_bad else rec.precision, rec.batch, m._state,
                                        force_grid=rec.force_grid)
                for dst, src in zip(rec.out, out):
                    dst.copy_(src)
                tot = dict(m.last_counts)
                m.overflow_rerenders += int(over)
            counts.append(tot)
        m.last_counts = counts[-1]
        return counts


def with_h2_fallback(model, precision, events, run):
    """run(precision, first) -> outputs, once; a fp32h2 run whose activations left the f16 range (the
    launches' range flag, one 4-byte read) blocks h2 for these weights, drops the events the run appended
    and runs again on fp32x3 (first False: without the caller's reuse_p1)."""
    n_ev = len(events) if events is not None else 0
    out = run(precision, True)
    if precision == "fp32h2" and not model.aggregator.h2_range_ok():
        model._block_h2()
        if events is not None:
            del events[n_ev:]
        out = run("fp32x3", False)
    return out


class _RenderState:
    """Device buffers one render stream reuses: the query buffers, the aggregate scratch and the P1 table
    (prepared model state like the packs and the grid, valid while p1_key matches)."""

    def __init__(self):
        self.p1 = None              # fp32 paths: P1 table [n_points, 256] (p1_table)
        self.p1_key = None          # what it was computed from; None: absent
        self.p1_builds = 0          # P1 builds launched on it (tests, tools)
        self.bufs = None            # launch-stream query buffers (query_chunk)
        self.qring = [None, None]   # query-stream buffer sets, used in turn (query_chunk)
        self.qfree = [None, None]   # per set: event behind its last launch-stream reader (record_chunk)
        self.qslot = 1              # the set the last query-stream query used (query_chunk)
        self.q_xkey = None          # points (storage, version) the query stream last saw (prepare)
        self.scratch, self.scratch_rows = None, 0   # aggregate scratch, the rows it was allocated for (scratch)
        self.scratch_key = None     # bf16: what the P1 at its head was computed from; None: partial or absent
        self.side = None            # fp32h2: the side stream P1 runs on (start_p1_side)
        self.used_bufs, self.used_n = None, None   # bf16: used_points_buffers for used_n points (aggregate_chunk)
        self.feat = None            # decoded features [rows, 129], reused by every call on this stream (feat_rows)
        self.feat_h = None          # bf16: the same as bf16 rows [rows, L.FEAT_H_PITCH] (feat_h_rows)
        self.pq_build = None        # render_pixels: the perspective query's build tables (_PixelCall.prepare)
        self.ray_hit = self.sample_dir = None   # render_pixels: the querier's ray mask, the samples' directions

    def _grown(self, name, rows, cols, dtype, dev):
        rows = max(int(rows), 1)
        buf = getattr(self, name)
        if buf is None or buf.shape[0] < rows or buf.device != dev:
            grown = max(rows, int(1.5 * (0 if buf is None else buf.shape[0])))
            buf = None
            setattr(self, name, None)   # the old rows are freed before the larger allocation
            setattr(self, name, torch.empty((grown, cols), dtype=dtype, device=dev))
        return getattr(self, name)[:rows]

    def feat_rows(self, rows: int, dev) -> torch.Tensor:
        """[rows, 129] view of the persistent feature buffer.  The calls of one stream use it in stream
        order (a call's composite reads it before the next call's aggregate writes it), so it is allocated
        once and grown by 1.5x: a multi-GB allocation inside a frame stalls the launch queue (c5: 20 GB
        per frame)."""
        return self._grown("feat", rows, 129, torch.float32, dev)

    def feat_h_rows(self, rows: int, dev) -> torch.Tensor:
        """feat_rows for pnr_aggregate_fwd_bf16_hf's bf16 feature rows."""
        return self._grown("feat_h", rows, L.FEAT_H_PITCH, torch.int16, dev)


# precision -> (entry point and the name L.check reports, the aggregator's pack, its extra split pack)
_AGGREGATE = {
    "fp32": ("pnr_aggregate_fwd", "packed", None),
    "fp32x3": ("pnr_aggregate_fwd_x3", "packed", "packed_x3"),
    "fp32h2": ("pnr_aggregate_fwd_h2", "packed", "packed_h2"),
    "bf16": ("pnr_aggregate_fwd_bf16", "packed_bf16", None),   # with bf16 feature rows: its _hf variant
}


def p1_per_frame() -> bool:
    """PNR_P1_PER_FRAME=1: every render call builds P1 again unless the caller passes reuse_p1 (what every
    call did before P1 became model state): the A/B switch of DESIGN §36 and a route test, in the manner of
    PNR_H2_GENERAL.  Read once per call."""
    return os.environ.get("PNR_P1_PER_FRAME") == "1"


class _RenderCall:
    """One render call.  capacity (every mode but EAGER): valid samples per ray the feature buffer is
    sized for, instead of a host read of each chunk's count; the counts then travel in the record."""

    def __init__(self, model, mode, precision, batch, state, force_grid=False, events=None, reuse_p1=False,
                 capacity=None, query_stream=None):
        self.m, self.mode, self.precision, self.batch, self.state = model, mode, precision, batch, state
        self.force_grid, self.events, self.reuse_p1 = force_grid, events, reuse_p1
        self.capacity, self.qs, self.bf16 = capacity, query_stream, precision == "bf16"
        self.p1_built, self.p1_per_frame = False, p1_per_frame()
        self.dev, self.R = batch.raydir.device, batch.raydir.shape[0]
        self.chunk = max(1, model.chunk_rays or self.R)   # rays per chunk
        self.n_chunks = max(1, -(-self.R // self.chunk))

    def run(self):
        self.prepare()
        p1_side = self.start_p1_side()
        for ci, r0 in enumerate(range(0, self.R, self.chunk)):
            r1 = min(self.R, r0 + self.chunk)
            rd, rc = self.chunk_rays(r0, r1)
            bufs, rays, qp = self.query_chunk(rd, rc)
            Sv, feat = self.size_chunk(bufs, r1 - r0)
            e2 = self.mark()
            s = self.samples(bufs, rd, Sv, rc)
            feat = self.aggregate_chunk(bufs, s, feat, Sv, p1_side)
            e3 = self.mark()
            self.composite_chunk(bufs, rays, qp, feat, Sv, r0, r1)
            self.record_chunk(ci, bufs)
            if self.events is not None:
                self.events += [("aggregate", e2, e3), ("composite", e3, self.mark())]
        return self.out, self.record()

    def mark(self, stream=None):
        if self.events is not None:   # else None
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            return e

    def prepare_outputs(self):
        """The call's output tensors, its background and its launch stream."""
        m, dev = self.m, self.dev
        self.C = C = m.aggregator.C          # 128 (fork) or 3 (upstream RGB head)
        f32 = dict(dtype=torch.float32, device=dev)
        self.out = (torch.empty((self.R, C), **f32), torch.empty((self.R, m.opt.SR), **f32),
                    torch.empty((self.R,), **f32), torch.empty((self.R,), dtype=torch.int8, device=dev))
        self.bg = bg_channels(self.batch.bg_color, C, dev)
        self.launch = torch.cuda.current_stream(dev)

    def prepare_tables(self):
        """The precision's packs, the points table (camera tables set), where the counts go."""
        m, dev = self.m, self.dev
        self.entry, pack, extra = _AGGREGATE[self.precision]
        self.mlp, keepw = getattr(m.aggregator, pack)()
        self.extra, keepx = getattr(m.aggregator, extra)() if extra else (None, None)
        self.packs = (self.mlp, keepw, self.extra, keepx)
        self.range_flag = keepx["range_flag"] if self.precision == "fp32h2" else None
        self.hf = self.bf16 and self.C == 128 and m.bf16_features
        self.pts, self._keep_pts = m.neural_points.tables(self.campos, self.camrot, bf16=self.bf16)
        self.totals = dict(S_filled=0, S_valid=0, R_hit=0, R_valid=0, n_pairs=0, n_cand=0)
        self.caps = []
        where = dict(pin_memory=True) if self.mode.counts == "pinned" else dict(device=dev)
        self.counts = None if self.mode.counts == "now" else torch.empty((self.n_chunks, 8), dtype=torch.int32, **where)

    def prepare(self):
        """Outputs, background, camera tables, the precision's packs, the points table, where the counts go."""
        m, b, st, dev = self.m, self.batch, self.state, self.dev
        L.require_gpu(b.raydir)
        if self.force_grid:   # a write the versions did not see: the grid and P1 are both stale
            m.neural_points.querier.grid.key = None
            st.p1_key = st.scratch_key = None
        self.prepare_outputs()
        if self.qs is not None:
            # the points can change on the launch stream (an optimizer step on xyz, a forced rebuild):
            # the query stream then waits for it before the grid build reads them
            xyz = m.neural_points.xyz
            xkey = (xyz.data_ptr(), xyz._version)
            if self.force_grid or st.q_xkey != xkey:
                self.qs.wait_stream(self.launch)
            st.q_xkey = xkey
        # the call's own copies of its inputs are made on the stream that queries (the caller makes the
        # inputs themselves ready there); without a query stream the context changes nothing
        with torch.cuda.stream(self.qs):
            self.campos, self.camrot = Q.camera_tables(b.campos, b.camrot, b.ray_cam)
            self.ray_cam = None if b.ray_cam is None else b.ray_cam.to(device=dev, dtype=torch.int32).contiguous()
        if self.qs is not None:
            # np_.tables and the aggregate read the camera tables on the launch stream (the query stream's
            # tail is the previous query, which the launch stream already waited for: no overlap is lost)
            self.launch.wait_stream(self.qs)
            for t in (self.campos, self.camrot, self.ray_cam):
                if t is not None:
                    t.record_stream(self.launch)
        self.prepare_tables()

    def start_p1_side(self):
        """fp32h2: block1.0's per-point half (P1) depends on the points and weights only, so it is built
        once into the state's table (p1_table) and again only when its key changes; a build runs on a
        side stream beside the query (which is latency bound and leaves the MFMA pipes idle) instead of in
        front of k_pairs_h2, and the aggregate waits on the returned event.  Only in the modes that do not
        read the counts before the aggregate, and not under capture (mode.side_p1); and only while P1 is
        the smaller job: P1 costs ~0.5 us per point, the query ~3.5 us per ray --
        measured 0.99 vs 2.25 ms at 2 M points / 640 k rays; at 10 M points / 1.25 M rays the 5.8 ms P1
        outlasted the query and the overlap gained nothing."""
        m, st, dev = self.m, self.state, self.dev
        if not (self.precision == "fp32h2" and self.mode.side_p1 and m.p1_side_stream
                and self.pts.n <= m.p1_side_max_points_per_ray * self.R):
            return None
        tab, ready0 = self.p1_table()
        if ready0:
            # built by an earlier call from these same points and weights: no launch.  The call's "p1"
            # stage is still recorded, empty: the stage lines of a sync-free fp32h2 call keep their names
            if self.events is not None:
                self.events.append(("p1", self.mark(), self.mark()))
            return None
        if st.side is None:
            st.side = torch.cuda.Stream(device=dev)
        st.side.wait_stream(torch.cuda.current_stream(dev))   # the launch stream's readers of the old table
        s0 = self.mark(st.side)
        L.check(L.lib().pnr_point_pre_h2(L.ctypes.byref(self.pts), L.ctypes.byref(self.extra), L.ptr(tab),
                                         tab.numel() * 4, L.c_void_p(st.side.cuda_stream)), "pnr_point_pre_h2")
        s1 = self.mark(st.side)
        ev_p1 = st.side.record_event()
        st.p1.record_stream(st.side)
        self.p1_built_now()
        if self.events is not None:
            self.events.append(("p1", s0, s1))
        return ev_p1

    def chunk_rays(self, r0, r1):
        """The chunk's contiguous directions (a copy of them belongs to the stream that queries) and cameras."""
        with torch.cuda.stream(self.qs):
            rd = self.batch.raydir[r0:r1].contiguous()
        if self.qs is not None:
            rd.record_stream(self.launch)
        return rd, None if self.ray_cam is None else self.ray_cam[r0:r1]

    def query_chunk(self, rd, rc):
        """The chunk's query -> bufs, rays, qp, ordered before what the launch stream does next.  On a
        query stream: two buffer sets in turn, each reused after the launch-stream work that read it."""
        st, b, np_, qs = self.state, self.batch, self.m.neural_points, self.qs
        if qs is not None:
            slot = st.qslot = st.qslot ^ 1
            if st.qfree[slot] is not None:
                qs.wait_event(st.qfree[slot])
        with torch.cuda.stream(qs):
            e0 = self.mark()
            bufs, _hp, rays, qp = np_.querier.run(np_.xyz.detach(), rd, self.campos, self.camrot, b.near, b.far,
                                                  bufs=st.bufs if qs is None else st.qring[slot], ray_cam=rc)
            if self.events is not None:
                self.events.append(("query", e0, self.mark()))
        if qs is None:
            st.bufs = bufs
        else:
            st.qring[slot] = bufs
            torch.cuda.current_stream(self.dev).wait_stream(qs)
        return bufs, rays, qp

    def samples(self, bufs, rd, Sv, rc):
        """pnr_samples of the chunk's valid samples, with room for Sv rows."""
        return bufs.samples(rd, Sv, rc)

    def size_chunk(self, bufs, n_rays):
        """The chunk's feature rows (its valid samples, read now, or what the capacity allows) and their buffer."""
        if self.mode.counts == "now":
            cnt = bufs.read_counts()
            for k in self.totals:
                self.totals[k] += cnt[k]
            self.m._queue.observe(cnt, n_rays)
            Sv = cnt["S_valid"]
        else:
            Sv = min(int(n_rays * self.capacity) + 1024, n_rays * self.m.opt.SR)
            self.caps.append((Sv, n_rays))
        return Sv, (self.state.feat_h_rows if self.hf else self.state.feat_rows)(Sv, self.dev)

    def p1_key(self):
        """What P1 depends on: the precision's kernel, the point count, and the storage and version of the
        embedding and of block1.0 (an in-place change bumps _version; the grid's contract)."""
        emb = self.m.neural_points.points_embeding
        b1 = self.m.aggregator.block1[0]
        # fp32h2 computes P1 on f16-split MFMA (k_point_pre_h2), the other fp32 paths on fp32 MFMA
        return (self.bf16, self.precision == "fp32h2", self.pts.n, emb.data_ptr(), emb._version, b1.weight.data_ptr(),
                b1.weight._version, b1.bias.data_ptr(), b1.bias._version)

    def p1_fresh(self, key_now):
        """The P1 a key speaks of may be taken as it is: the key is the call's, and the call is neither one
        that builds its own (the captured graph, PNR_P1_PER_FRAME=1 without the reuse_p1 hint) nor still
        before its build."""
        own = self.mode is CAPTURE or (self.p1_per_frame and not self.reuse_p1)
        return key_now == self.p1_key() and (self.p1_built or not own)

    def p1_table(self):
        """The fp32 paths' P1 table -> (the table, P1 already valid).  An allocation of the render
        state's own, [n_points, 256] (the p1_table of the pnr_aggregate_fwd*_p1 calls), made once per point
        count and device: the scratch's growth leaves it alone.  Valid while the key it was built from is the call's."""
        st, dev, n = self.state, self.dev, int(self.pts.n)
        if st.p1 is None or st.p1.device != dev or st.p1.shape[0] != n:
            st.p1 = st.p1_key = None   # the old table is freed before the new allocation
            st.p1 = torch.empty((n, 256), dtype=torch.float32, device=dev)
        return st.p1, self.p1_fresh(st.p1_key)

    def p1_built_now(self):
        """A full P1 build into the state's table (bf16: the scratch's start) was just launched."""
        st = self.state
        if self.bf16:
            st.scratch_key = self.p1_key()
        else:
            st.p1_key = self.p1_key()
        self.p1_built = True
        st.p1_builds += 1

    def scratch(self, n_max):
        """Persistent aggregate scratch -> (tensor, P1 already valid).  The fp32 paths keep P1 in p1_table;
        bf16 keeps its bf16 P1 rows at the scratch's start (pnr_points.p1_ready), valid by the same key
        until the scratch grows."""
        st, dev = self.state, self.dev
        n_points = int(self.pts.n) if self.bf16 else 0
        # the one size query that allocates nothing: the persistent scratch is kept while it is large enough
        query = "pnr_aggregate_scratch_bytes_bf16" if self.bf16 else "pnr_aggregate_scratch_bytes"
        nb = L.c_size_t(0)
        L.check(getattr(L.lib(), query)(int(n_max), n_points, L.ctypes.byref(nb)), query)
        if st.scratch is None or st.scratch.device != dev or st.scratch.numel() * 4 < int(nb.value):
            # headroom (n_max varies per batch) and geometric growth: no allocation per frame
            st.scratch_rows = max(int(n_max * 1.5) + 1024, int(1.5 * st.scratch_rows))
            st.scratch = st.scratch_key = None
            st.scratch = L.scratch(query, st.scratch_rows, n_points, device=dev).view(torch.float32)
        if not self.bf16:
            st.scratch_key = None   # the scratch's start is this call's hid rows now
            return st.scratch, self.p1_table()[1]
        return st.scratch, self.p1_fresh(st.scratch_key)

    def aggregate_chunk(self, bufs, s, feat, Sv, p1_side):
        """The precision's aggregate into feat (-> the rows the composite reads), P1 as it stands if valid."""
        m, st, pts, dev = self.m, self.state, self.pts, self.dev
        scratch, ready = self.scratch(max(Sv, 1))
        # bf16 (config c5: 20 M points, a frame references a fraction of them): block1.0's point half only
        # for the points this batch's neighbour lists reference (pnr_used_points, device list and count),
        # written at their own rows of the P1 table (pnr_points.used without used_map) -- no indirection
        # in the pairs kernel.  (A reuse_p1 call after a used-only one finds the table partial (key
        # cleared): it computes its own used rows, not the whole table.)
        partial = self.bf16 and self.mode.used_only and m.p1_used_only and self.n_chunks == 1 and not ready
        if partial:
            if st.used_n != pts.n:
                st.used_bufs, st.used_n = used_points_buffers(pts.n, dev), pts.n
            pts.used = L.ptr(used_points_device(bufs, m.opt.K, pts.n, st.used_bufs)[0])
            pts.n_used, pts.used_map = pts.n, None
            pts.n_used_dev = bufs.count_ptr(Q.COUNT_N_USED)
            st.scratch_key = None   # the table holds this batch's rows only
        if p1_side is not None:   # P1 written into the table by the side stream
            torch.cuda.current_stream(dev).wait_event(p1_side)
        elif not ready and not partial and Sv > 0:
            # this launch builds it, in front of the pairs kernel (a call without samples launches nothing)
            self.p1_built_now()
        pts.p1_ready = int(ready)
        # the fp32 paths: the entry point's _p1 form, P1 in the state's table behind the packs
        fn = getattr(L.lib(), self.entry + (("_hf" if self.hf else "") if self.bf16 else "_p1"))
        extra = () if self.extra is None else (L.ctypes.byref(self.extra),)
        extra += () if self.bf16 else (L.ptr(st.p1),)
        L.check(fn(L.ctypes.byref(pts), L.ctypes.byref(s), L.ctypes.byref(self.mlp), *extra, L.ptr(feat), None, None,
                   L.ptr(scratch), scratch.numel() * 4, L.stream_ptr(dev)), self.entry)
        if self.C == 3:   # upstream colour head: [alpha, rgb] rows
            feat = m.aggregator.apply_rgb_head(feat, n_dev=bufs.counts[1:2], n=Sv)
        return feat

    def composite_chunk(self, bufs, rays, qp, feat, Sv, r0, r1):
        opt = self.m.opt
        cp = L.CompositeParams(float(opt.vsize[2]), int(opt.raydist_mode_unit), self.C, L.ptr(self.bg), max(Sv, 1))
        comp = L.lib().pnr_composite_fwd_hf if self.hf else L.lib().pnr_composite_fwd
        L.check(comp(L.ctypes.byref(rays), L.ctypes.byref(qp), L.ctypes.byref(bufs.c), L.ctypes.byref(cp), L.ptr(feat),
                     *(L.ptr(t[r0:r1]) for t in self.out), L.stream_ptr(self.dev)), "pnr_composite_fwd")

    def record_chunk(self, ci, bufs):
        """The chunk's counts on their way, and its query-buffer set handed back."""
        if self.counts is not None:
            self.counts[ci].copy_(bufs.counts, non_blocking=self.mode.counts == "pinned")
        if self.qs is not None:   # the launch stream's last reader of this query-buffer set
            self.state.qfree[self.state.qslot] = torch.cuda.current_stream(self.dev).record_event()

    def record(self):
        """EAGER: the call's counts become last_counts.  Else what finish() / RenderGraph.check() must still see."""
        m = self.m
        if self.mode.counts == "now":
            m.last_counts = self.totals
            return None
        range_host = event = None
        if self.mode.counts == "pinned":
            if self.range_flag is not None:
                # the fp32h2 range flag as it stands after this call's launches, to pinned memory behind the
                # call's event: finish() reads it without a stream sync (which would wait for later calls)
                range_host = torch.empty(1, dtype=torch.int32, pin_memory=True)
                range_host.copy_(self.range_flag, non_blocking=True)
            event = torch.cuda.current_stream().record_event()
        return _PendingCall(self.precision, self.caps, self.counts, self.range_flag, range_host, event, self.batch,
                            self.force_grid, self.out, m.aggregator.h2_key(), m.neural_points.querier.grid.key,
                            self.packs if self.mode is CAPTURE else ())


class PixelBatch(namedtuple("PixelBatch", "campos camrot pixel_idx h w intrinsic near far bg_color")):
    """The inputs of one render_pixels call: pixel_idx int32 [R,2] on the device, h / w ints, intrinsic a
    numpy fp32 [3,3], near / far floats."""
    __slots__ = ()

    @classmethod
    def of(cls, dev, campos, camrot, pixel_idx, h, w, intrinsic, near, far, bg_color):
        """From a caller's arguments: tensors or numbers for h / w / near / far, the first intrinsic of a
        batch, and pixel_idx None for the whole h x w frame in row-major order."""
        h, w = L.host_scalar(h, int), L.host_scalar(w, int)
        intr = intrinsic.detach().cpu().numpy() if torch.is_tensor(intrinsic) else intrinsic
        if pixel_idx is None:
            ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.int32, device=dev),
                                    torch.arange(w, dtype=torch.int32, device=dev), indexing="ij")
            pix = torch.stack([xs, ys], -1).reshape(-1, 2).contiguous()
        else:
            pix = pixel_idx.to(dev).reshape(-1, 2).to(torch.int32).contiguous()
        return cls(campos, camrot, pix, h, w, np.asarray(intr, np.float32).reshape(-1, 3, 3)[0],
                   L.host_scalar(near, float, torch.min), L.host_scalar(far, float, torch.max), bg_color)


class _PixelCall(_RenderCall):
    """One render_pixels call: _RenderCall's stages on the perspective query.  The rays are
    pixels; the query is pnr_pquery_bufs on one pnr_pquery_build per call; the samples carry their own
    directions; the composite is pnr_composite_fwd_p.  EAGER only (one counts read per chunk)."""

    def __init__(self, model, precision, batch, state, events=None, reuse_p1=False):
        self.m, self.mode, self.precision, self.batch, self.state = model, EAGER, precision, batch, state
        self.force_grid, self.events, self.reuse_p1 = False, events, reuse_p1
        self.capacity, self.qs, self.bf16 = None, None, False
        self.p1_built, self.p1_per_frame = False, p1_per_frame()
        self.dev, self.R = batch.pixel_idx.device, batch.pixel_idx.shape[0]
        self.chunk = max(1, model.chunk_rays or self.R)
        self.n_chunks = max(1, -(-self.R // self.chunk))

    def prepare(self):
        """_RenderCall.prepare, plus the cloud's perspective coordinates (NeuralPoints.w2pers, the call the
        seam path makes, so both bin the same values) and the call's one query build."""
        m, b, st, dev = self.m, self.batch, self.state, self.dev
        np_, opt = m.neural_points, m.opt
        L.require_gpu(b.pixel_idx)
        self.prepare_outputs()
        self.campos, self.camrot = Q.camera_tables(b.campos, b.camrot)
        self.prepare_tables()
        xyz = np_.xyz.detach()
        self.pers = np_.w2pers(xyz, self.camrot[None], self.campos[None]).reshape(-1, 3).float().contiguous()
        self.pts.pers = L.ptr(self.pers)
        self.geo = geo = QP.frustum_geometry(opt, b.h, b.w, b.intrinsic, b.near, b.far)
        if int(geo.dims[2]) > 65535:
            raise L.PnrError(f"render_pixels: {int(geo.dims[2])} depth ids do not fit the query buffers (65535)")
        self.pq = QP.pquery_params(opt, geo)
        # the centre depth of fz = -1 (pnr_pquery's sample_loc of an unfilled slot)
        self.z_unfilled = float(np.float32(np.float64(geo.ranges[2]) - 0.5 * np.float64(geo.scaled_vsize[2])))
        self.qparams = query_params(opt.SR, opt.K)
        N = self.pers.shape[0]
        dims = (L.c_int32 * 3)(*[int(v) for v in geo.dims])
        nb = L.c_size_t(0)
        L.check(L.lib().pnr_pquery_scratch_bytes(N, 0, int(opt.SR), dims, L.ctypes.byref(nb)),
                "pnr_pquery_scratch_bytes")
        if st.pq_build is None or st.pq_build.device != dev or st.pq_build.numel() < int(nb.value):
            st.pq_build = None
            st.pq_build = torch.empty(-(-int(nb.value) // 16) * 16, dtype=torch.uint8, device=dev)
        self.pq_stats = torch.zeros(8, dtype=torch.int32, device=dev)
        self.ray_valid = torch.zeros(self.R, dtype=torch.bool, device=dev)
        e0 = self.mark()
        L.check(L.lib().pnr_pquery_build(L.ctypes.byref(self.pq), L.ptr(self.pers), N, L.ptr(self.pq_stats),
                                         L.ptr(st.pq_build), st.pq_build.numel(), L.stream_ptr(dev)),
                "pnr_pquery_build")
        if self.events is not None:
            self.events.append(("build", e0, self.mark()))

    def run(self):
        """_RenderCall.run; the outputs end with ray_valid ([R] bool: the ray has a valid sample)."""
        out, rec = super().run()
        return out + (self.ray_valid,), rec

    def chunk_rays(self, r0, r1):
        return self.batch.pixel_idx[r0:r1], None

    def query_chunk(self, pix, rc):
        st, dev = self.state, self.dev
        R, SR, K = pix.shape[0], int(self.m.opt.SR), int(self.m.opt.K)
        if st.bufs is None or not st.bufs.fits(R, SR, K) or st.bufs.counts.device != dev:
            st.bufs = Q.QueryBuffers(R, SR, K, dev)
        if (st.ray_hit is None or st.ray_hit.device != dev or st.ray_hit.shape[0] < max(R, 1)
                or st.sample_dir.shape[0] < max(R * SR, 1)):
            st.ray_hit = torch.empty(max(R, 1), dtype=torch.int8, device=dev)
            st.sample_dir = torch.empty((max(R * SR, 1), 3), dtype=torch.float32, device=dev)
        e0 = self.mark()
        L.check(L.lib().pnr_pquery_bufs(L.ctypes.byref(self.pq), self.pers.shape[0], L.ptr(pix), R, L.ptr(self.campos),
                                        L.ptr(self.camrot), L.ctypes.byref(st.bufs.c), L.ptr(st.ray_hit),
                                        L.ptr(st.sample_dir), L.ptr(st.pq_build), st.pq_build.numel(),
                                        L.stream_ptr(dev)), "pnr_pquery_bufs")
        if self.events is not None:
            self.events.append(("query", e0, self.mark()))
        return st.bufs, None, self.qparams

    def samples(self, bufs, pix, Sv, rc):
        """The samples carry their own directions (pers2w of the centre): dirs row = sample row."""
        return L.Samples(bufs.valid_list.data_ptr(), bufs.count_ptr(Q.COUNT_S_VALID), Sv, bufs.pidx.data_ptr(),
                         bufs.sample_w.data_ptr(), bufs.sample_p.data_ptr(), self.state.sample_dir.data_ptr(), None,
                         1, bufs.K, None)

    def composite_chunk(self, bufs, rays, qp, feat, Sv, r0, r1):
        cp = L.CompositeParams(float(self.geo.vsize[2]), int(self.m.opt.raydist_mode_unit), self.C, L.ptr(self.bg),
                               max(Sv, 1))
        L.check(L.lib().pnr_composite_fwd_p(L.ctypes.byref(qp), L.ctypes.byref(bufs.c), L.ctypes.byref(cp), r1 - r0,
                                            L.ptr(self.state.ray_hit), self.z_unfilled, L.ptr(feat),
                                            *(L.ptr(t[r0:r1]) for t in self.out), L.stream_ptr(self.dev)),
                "pnr_composite_fwd_p")
        torch.gt(bufs.ray_vcnt[:r1 - r0], 0, out=self.ray_valid[r0:r1])


class RenderGraph:
    """One ray batch's full render (query -> aggregate -> composite) captured in a HIP graph and replayed
    without any host work beyond the launch: SURVEY 8(f) rank 2 (the reference syncs at qpiw.py:656, 716
    and neural_points.py:786).  The graph owns its query buffers, aggregate scratch and outputs; the camera
    and ray directions are static input tensors that ``replay`` refreshes in place.  Capture requires an
    already built grid and fixed weights (the launches point at the current grid tables and weight packs;
    rebuild the graph after either changes).

    The feature buffer is sized from an eager render of the same batch (valid samples x ``margin``);
    ``check()`` reads the replay's counts and the fp32h2 range flag (one host sync) and returns False when
    the replay overflowed that size or an activation left the f16 range -- then render that frame with
    ``render_rays`` instead."""

    def __init__(self, model, campos, camrot, raydir, near, far, bg_color, margin: float = 1.25):
        L.require_gpu(raydir)
        self.model, dev = model, raydir.device
        self.campos = campos.reshape(3).float().to(dev).clone()
        self.camrot = camrot.reshape(3, 3).float().to(dev).clone()
        self.raydir = raydir.reshape(-1, 3).float().contiguous().clone()
        self.near, self.far = near, far
        bg = bg_channels(bg_color, model.aggregator.C, dev)
        self.bg = None if bg is None else bg.clone()
        batch = RayBatch(self.campos, self.camrot, self.raydir, near, far, self.bg)
        model._sync_rw2c()
        self.precision = model._precision_now()
        R = self.raydir.shape[0]
        chunk = max(1, model.chunk_rays or R)
        self.state = _RenderState()
        # eager render: builds nothing new (grid must exist), sizes the buffers
        model._render_rays(EAGER, self.precision, batch, self.state)
        self.eager_counts = dict(model.last_counts)
        cap = margin * max(self.eager_counts["S_valid"], 1) / max(min(chunk, R), 1)
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):   # warm-up on a side stream (allocations, packs)
            model._render_rays(WARMUP, self.precision, batch, self.state, capacity=cap)
        torch.cuda.current_stream(dev).wait_stream(stream)
        torch.cuda.synchronize(dev)
        # Nothing may issue a capture-illegal HIP call (hipFree, an event or stream sync) while the graph
        # records -- from this thread, or from a finaliser the garbage collector runs at some allocation
        # inside the capture (the GPUTEST_r04 failure).  Collect dead cycles now, keep the collector off
        # during the capture, and have GridHandle finalisers defer their frees (querier._DEFERRED); other
        # threads' calls cannot invalidate a thread-local capture.
        gc.collect()
        Q.release_deferred()
        gc_was_on = gc.isenabled()
        gc.disable()
        Q._CAPTURES[0] += 1
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.out, self.rec = model._render_rays(CAPTURE, self.precision, batch, self.state, capacity=cap)
        finally:
            Q._CAPTURES[0] -= 1
            if gc_was_on:
                gc.enable()
        Q.release_deferred()
        self.capacity = cap

    def replay(self, campos=None, camrot=None, raydir=None):
        """Render the batch again (new camera / rays copied into the static inputs first); returns
        (ray_color, opacity, is_bg, ray_mask), tensors the graph owns and overwrites on the next replay."""
        for static, new, shape in ((self.campos, campos, (3,)), (self.camrot, camrot, (3, 3)),
                                   (self.raydir, raydir, (-1, 3))):
            if new is not None:
                static.copy_(new.reshape(shape))
        self.graph.replay()
        return self.out

    def check(self) -> bool:
        """True when the last replay's outputs are valid: every chunk's valid samples fit the captured
        feature buffer and (fp32h2) no activation left the f16 range.  Synchronises."""
        ok = True
        for cap, _rays, c in chunk_counts(self.rec):
            self.last_counts = c
            ok &= c["S_valid"] <= cap
        if self.precision == "fp32h2" and not self.model.aggregator.h2_range_ok():
            self.model.aggregator.h2_reset_range()
            ok = False
        return ok
