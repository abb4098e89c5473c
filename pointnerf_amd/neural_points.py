"""The neural point cloud (moved out of renderer.py).

``NeuralPoints`` mirrors the parameter table of
models/neural_points/neural_points.py:11-331 (same parameter names, so the
``neural_points.*`` keys of a reference checkpoint load into it) and its
14-tuple ``forward`` (neural_points.py:782-812) for API compatibility.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from .querier import lighting_fast_querier
from .querier_p import lighting_fast_querier as lighting_fast_querier_p


class NeuralPoints(nn.Module):
    """Point table of neural_points.NeuralPoints; opt.wcoord_query picks the
    querier as neural_points.py:330 does: > 0 the world grid (querier.py), 0 the
    perspective frustum (querier_p.py)."""

    def __init__(self, opt, device, xyz=None, embedding=None, color=None, dirs=None, conf=None,
                 Rw2c=None, emb_dtype=torch.float32):
        """emb_dtype torch.bfloat16 stores points_embeding in bf16 (SURVEY config
        c5: 104 B per point instead of 168; the bf16 render path reads it
        directly, the fp32 paths from an fp32 copy; training needs fp32)."""
        super().__init__()
        if emb_dtype not in (torch.float32, torch.bfloat16):
            raise L.PnrError(f"emb_dtype {emb_dtype}: float32 or bfloat16")
        # row width of points_embeding: opt.point_features_dim (32 lego, 63 the DTU scripts)
        self.E = int(getattr(opt, "point_features_dim", 32))
        if emb_dtype == torch.bfloat16 and self.E != 32:
            raise L.PnrError(f"a bf16 embedding table needs point_features_dim 32, not {self.E} "
                             "(the bf16 aggregate is 32-wide only)")
        self.emb_dtype = emb_dtype
        self._emb32 = (None, None)
        self.opt = opt
        self.device = torch.device(device)
        self.xyz = nn.Parameter(torch.zeros((0, 3), device=self.device), requires_grad=False)
        self.points_embeding = nn.Parameter(torch.zeros((1, 0, self.E), device=self.device))
        self.points_conf = None
        self.points_dir = None
        self.points_color = None
        self.Rw2c = torch.eye(3, device=self.device)
        if xyz is not None:
            self.set_points(xyz, embedding, color, dirs, conf, Rw2c)
        self.perspective = getattr(opt, "wcoord_query", 1) <= 0
        self.querier = (lighting_fast_querier_p if self.perspective else lighting_fast_querier)(self.device, opt)

    def set_points(self, xyz, embedding, color=None, dirs=None, conf=None, Rw2c=None):
        """set_points (neural_points.py:480-546) with point_*_mode '1'; xyz is
        trainable with --xyz_grad 1 (neural_points.py:270: the HIP backward's
        pnr_aggregate_bwd_xyz, render_rays_train only)."""
        dev = self.device
        if embedding.shape[-1] != self.E:
            raise L.PnrError(f"embedding table is {embedding.shape[-1]} wide, point_features_dim is {self.E} "
                             "(NeuralPoints.assemble_embedding builds the table of a DTU flag set)")
        self.xyz = nn.Parameter(xyz.to(dev).float().reshape(-1, 3).contiguous(),
                                requires_grad=getattr(self.opt, "xyz_grad", 0) > 0)
        self.points_embeding = nn.Parameter(embedding.to(dev).to(self.emb_dtype).reshape(1, -1, self.E).contiguous())
        self.points_color = None if color is None else nn.Parameter(color.to(dev).float().reshape(1, -1, 3).contiguous())
        self.points_dir = None if dirs is None else nn.Parameter(dirs.to(dev).float().reshape(1, -1, 3).contiguous())
        self.points_conf = None if conf is None else nn.Parameter(conf.to(dev).float().reshape(1, -1, 1).contiguous())
        # [3,3] uniform, or [N,3,3] per point (neural_points.py:289, 799; pnr_points.rw2c)
        self.Rw2c = torch.eye(3, device=dev) if Rw2c is None else Rw2c.to(dev).float().contiguous()
        if self.Rw2c.dim() == 3 and self.Rw2c.shape != (self.xyz.shape[0], 3, 3):
            raise L.PnrError(f"per-point Rw2c must be [N,3,3], got {tuple(self.Rw2c.shape)}")

    @staticmethod
    def assemble_embedding(opt, feat, color=None, dirs=None, conf=None):
        """The point tables of set_points (neural_points.py:480-540) from a cloud's parts: feat [N,F]
        truncated to point_features_dim, conf replaced by default_conf when that is in (0, 1], then conf,
        dir and colour prepended -- in that order, so the row is [colour, dir, conf, feat] -- for each
        point_*_mode containing "0"; a part stays a table of its own for each mode containing "1".
        Returns (embedding [1,N,E], color, dirs, conf), the constructor's arguments.  The assembled width
        must be point_features_dim; a colour or dir mode without "1" would take block3.0's inputs away
        (no reference script does it) and is refused."""
        E = int(getattr(opt, "point_features_dim", 32))
        emb = feat.reshape(-1, feat.shape[-1]).float()[:, :E]
        n = emb.shape[0]
        dc = float(getattr(opt, "default_conf", -1.0))
        if conf is not None and 0.0 < dc <= 1.0:
            conf = torch.full((n, 1), dc, dtype=torch.float32, device=emb.device)
        kept = {}
        for name, part, width in (("conf", conf, 1), ("dir", dirs, 3), ("color", color, 3)):
            mode = str(getattr(opt, f"point_{name}_mode", "1"))
            kept[name] = None
            if part is None:
                continue
            part = part.reshape(n, width).float().to(emb.device)
            if name != "conf" and "1" not in mode:
                raise L.PnrError(f"point_{name}_mode {mode!r}: without '1' block3.0 loses its {name} inputs; "
                                 "not implemented by libpnr")
            if "0" in mode:
                emb = torch.cat([part, emb], dim=-1)
            if "1" in mode:
                kept[name] = part
        if emb.shape[-1] != E:
            raise L.PnrError(f"assembled embedding is {emb.shape[-1]} wide (features {min(feat.shape[-1], E)} + the "
                             f"parts with a '0' mode), point_features_dim is {E}")
        return emb.reshape(1, n, E).contiguous(), kept["color"], kept["dir"], kept["conf"]

    def embedding_fp32(self) -> torch.Tensor:
        """points_embeding as fp32 [N,E] (the table itself, or a copy of the bf16
        table cached on its storage and version)."""
        e = self.points_embeding.detach().reshape(-1, self.E)
        if e.dtype == torch.float32:
            return e.contiguous()
        key = (e.data_ptr(), self.points_embeding._version, e.shape[0])
        if self._emb32[0] != key:
            self._emb32 = (key, e.float().contiguous())
        return self._emb32[1]

    def tables(self, campos=None, camrot=None, bf16: bool = False) -> tuple[L.Points, tuple]:
        """pnr_points of the table; bf16 (the bf16 aggregate) passes a bf16
        embedding table as emb_bf16 instead of an fp32 one."""
        e = self.points_embeding.detach().reshape(-1, self.E)
        use_b = bf16 and e.dtype == torch.bfloat16
        if bf16 and self.E != 32:
            raise L.PnrError(f"the bf16 aggregate and the probe need point_features_dim 32, not {self.E}")
        keep = (self.xyz.detach().contiguous(), None if use_b else self.embedding_fp32(),
                None if self.points_color is None else self.points_color.detach().reshape(-1, 3).contiguous(),
                None if self.points_dir is None else self.points_dir.detach().reshape(-1, 3).contiguous(),
                None if self.points_conf is None else self.points_conf.detach().reshape(-1).contiguous(),
                e.contiguous() if use_b else None)
        p = L.Points(keep[0].shape[0], keep[0].data_ptr(), None, L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]),
                     L.ptr(keep[4]), L.ptr(campos), L.ptr(camrot))
        p.emb_bf16 = L.ptr(keep[5])
        p.emb_dim = self.E
        rw = self.rw2c_table()
        p.rw2c = L.ptr(rw)
        return p, keep + (rw,)

    def rw2c_table(self):
        """The per-point Rw2c as the kernels read it ([N,9] fp32), or None for a
        uniform Rw2c (that one goes through the aggregator's pnr_mlp.rw2c)."""
        rw = self.Rw2c
        if rw is None or rw.dim() == 2:
            return None
        if rw.shape[0] != self.xyz.shape[0]:
            raise L.PnrError(f"per-point Rw2c has {rw.shape[0]} rows, the cloud {self.xyz.shape[0]} points")
        return rw.detach().reshape(-1, 9).float().contiguous()

    def bytes_per_point(self) -> int:
        """HBM bytes of one point's parameters (168 fp32, 104 with a bf16 embedding)."""
        b = 12 + self.E * self.points_embeding.element_size()
        for t, c in ((self.points_color, 3), (self.points_dir, 3), (self.points_conf, 1)):
            if t is not None:
                b += c * t.element_size()
        return b

    def w2pers(self, point_xyz, camrotc2w, campos):
        """neural_points.py:687-693."""
        point_xyz_shift = point_xyz[None, ...] - campos[:, None, :]
        xyz = torch.sum(camrotc2w[:, None, :, :] * point_xyz_shift[:, :, :, None], dim=-2)
        return torch.stack([xyz[:, :, 0] / xyz[:, :, 2], xyz[:, :, 1] / xyz[:, :, 2], xyz[:, :, 2]], dim=-1)

    def forward(self, inputs):
        """neural_points.py:782-812: query + gather, returns the 14-tuple the
        reference PointAggregator consumes (API path; the fused renderer does
        the gather inside pnr_aggregate_fwd instead)."""
        camrotc2w, campos = inputs["camrotc2w"], inputs["campos"]
        near, far = inputs["near"], inputs["far"]
        pers = self.w2pers(self.xyz, camrotc2w, campos)
        pixel_idx = inputs.get("pixel_idx")
        if self.perspective:
            for name in ("pixel_idx", "h", "w", "intrinsic"):
                if inputs.get(name) is None:
                    raise L.PnrError(f"NeuralPoints.forward with wcoord_query 0 (the perspective query) needs "
                                     f"inputs[{name!r}]")
            pixel_idx = pixel_idx.to(torch.int32)
        (sample_pidx, sample_loc, sample_loc_w, sample_ray_dirs, ray_mask, vsize, ranges) = \
            self.querier.query_points(pixel_idx, pers, self.xyz[None, ...], None,
                                      inputs.get("h"), inputs.get("w"), inputs.get("intrinsic"),
                                      L.host_scalar(near, float, torch.min), L.host_scalar(far, float, torch.max),
                                      inputs["raydir"], campos, camrotc2w)
        mask = sample_pidx >= 0
        B, R, SR, K = sample_pidx.shape
        idx = torch.clamp(sample_pidx, min=0).view(-1).long()
        cat = torch.cat([self.xyz[None, ...], pers, self.points_embeding.float()], dim=-1)
        g = torch.index_select(cat, 1, idx).view(B, R, SR, K, cat.shape[-1])

        def sel(t, c):
            return None if t is None else torch.index_select(t, 1, idx).view(B, R, SR, K, c)

        rw = self.Rw2c if self.Rw2c.dim() == 2 else torch.index_select(self.Rw2c, 0, idx).view(B, R, SR, K, 3, 3)
        return (sel(self.points_color, 3), rw, sel(self.points_dir, 3), sel(self.points_conf, 1),
                g[..., 6:], g[..., 3:6], g[..., :3], mask, sample_loc, sample_loc_w, sample_ray_dirs,
                ray_mask, vsize, 0)
