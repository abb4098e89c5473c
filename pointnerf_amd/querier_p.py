"""Perspective-frustum neural-point querier (--wcoord_query 0) on libpnr.so.

``lighting_fast_querier`` here is the drop-in for the reference's
models/neural_points/query_point_indices.py:34-116 (seam 1): the
same constructor, ``clean_up``, ``get_hyperparameters(h, w, intrinsic, near,
far)`` and 12-argument ``query_points`` returning the same 7-tuple.  The query
itself is ``pnr_pquery`` (csrc/pquery.hip); ``pers2w`` and the training jitter
are torch ops on the compacted [1,R',SR,3] tensor.  One host read per call: R'.

``frustum_geometry`` is plain numpy and importable without a GPU.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L

JITTERS = ("passfunc", "uniform", "gaussian")


def resolved_query_size(opt):
    """opt.query_size, or kernel_size when it is left at (0, 0, 0) (neural_points.py:329)."""
    qs = list(getattr(opt, "query_size", (0, 0, 0)))
    return [int(v) for v in (opt.kernel_size if qs[0] == 0 else qs)]


def check_sizes(opt):
    """The walk of a sample must stay inside the query_size block marked round
    the sample's own voxel: with a wider kernel the reference's neighbours of a
    ray depend on which other rays share its batch."""
    ks, qs = [int(v) for v in opt.kernel_size], resolved_query_size(opt)
    hx = (ks[0] + 1) // 2 - 1
    hz = min(hx, (ks[2] + 1) // 2 - 1)
    if hx > (qs[0] + 1) // 2 - 1 or hx > (qs[1] + 1) // 2 - 1 or hz > (qs[2] + 1) // 2 - 1:
        raise L.PnrError(f"perspective query: kernel_size {ks} is wider than query_size {qs}; the reference's result "
                         "then depends on the other rays of the batch, which is not reproduced")


def check_supported(opt):
    """What every entry of the perspective query refuses (the querier, frustum_geometry, render_pixels),
    stated once."""
    if getattr(opt, "inverse", 0):
        raise L.PnrError("--inverse 1 (disparity ray generation) is not supported")
    if int(getattr(opt, "NN", 2)) <= 0:
        raise L.PnrError("NN == 0 (query_rand_along_ray: a reservoir seeded by time()) is not supported")
    check_sizes(opt)
    jitter = getattr(opt, "shpnt_jitter", "passfunc")
    if jitter not in JITTERS:
        raise L.PnrError(f"shpnt_jitter {jitter!r}: one of {JITTERS}")
    return jitter


def frustum_geometry(opt, h, w, intrinsic, near_depth, far_depth):
    """get_hyperparameters (query_point_indices.py:52-75) in numpy with the
    reference's promotions for an fp32 intrinsic and fp32 depths: ranges,
    vsize, vdim, vscale, dims (scaled_vdim), scaled_vsize, ray_vsize,
    radius_limit, depth_limit."""
    check_supported(opt)
    k = np.asarray(intrinsic, dtype=np.float32).reshape(3, 3)
    h, w = int(np.asarray(h).reshape(-1)[0]), int(np.asarray(w).reshape(-1)[0])
    near, far = np.float32(np.asarray(near_depth).reshape(-1)[0]), np.float32(np.asarray(far_depth).reshape(-1)[0])
    x_rl, x_rh = -k[0, 2] / k[0, 0], (np.float32(w) - k[0, 2]) / k[0, 0]
    y_rl, y_rh = -k[1, 2] / k[1, 1], (np.float32(h) - k[1, 2]) / k[1, 1]
    ranges = np.array([x_rl, y_rl, near, x_rh, y_rh, far], dtype=np.float32)
    vdim = np.array([w, h, opt.z_depth_dim], dtype=np.int32)
    # an fp32 scalar over an int32 one is an fp64 quotient; the array rounds it to fp32
    vsize = np.array([np.float64(x_rh - x_rl) / vdim[0], np.float64(y_rh - y_rl) / vdim[1],
                      np.float64(far - near) / vdim[2]], dtype=np.float32)
    vscale = np.array(opt.vscale, dtype=np.int32)
    dims = np.ceil(vdim / vscale).astype(np.int32)
    scaled_vsize = (vsize * vscale).astype(np.float32)
    ray_vsize = (scaled_vsize / vscale).astype(np.float32)
    radius_limit = np.float32(np.float32(opt.radius_limit_scale) * max(vsize[0], vsize[1]))
    depth_limit = np.float32(np.float32(opt.depth_limit_scale) * vsize[2])
    return SimpleNamespace(ranges=ranges, vsize=vsize, vdim=vdim, vscale=vscale, dims=dims, scaled_vsize=scaled_vsize,
                           ray_vsize=ray_vsize, radius_limit=radius_limit, depth_limit=depth_limit, h=h, w=w)


def pquery_params(opt, geo) -> L.PQueryParams:
    q = L.PQueryParams()
    q.shift[:] = [float(v) for v in geo.ranges[:3]]
    q.scaled_vsize[:] = [float(v) for v in geo.scaled_vsize]
    q.ray_vsize[:] = [float(v) for v in geo.ray_vsize]
    q.dims[:] = [int(v) for v in geo.dims]
    q.vscale[:] = [int(v) for v in geo.vscale]
    q.w, q.h = geo.w, geo.h
    q.SR, q.K, q.P, q.NN = int(opt.SR), int(opt.K), int(opt.P), int(opt.NN)
    q.kernel_size[:] = [int(v) for v in opt.kernel_size]
    q.query_size[:] = resolved_query_size(opt)
    q.radius_limit2 = float(np.float32(geo.radius_limit ** 2))   # np.float32(radius_limit ** 2), :752
    q.depth_limit2 = float(np.float32(geo.depth_limit ** 2))
    q.grid_seed = int(getattr(opt, "grid_seed", 0))
    return q


class lighting_fast_querier:  # noqa: N801  (reference class name)
    """query_point_indices.lighting_fast_querier on libpnr.so."""

    def __init__(self, device, opt):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        if self.device.type != "cuda":
            raise L.PnrError("lighting_fast_querier needs a cuda (ROCm) device")
        self.gpu = self.device.index or 0
        self.opt = opt
        check_supported(opt)
        self.inverse = getattr(opt, "inverse", 0)
        self.count = 0
        self.last_slot_z = None     # [R',SR] int32: the depth ids of the last call's samples
        self._stats_dev = None

    def clean_up(self):
        self.last_slot_z = self._stats_dev = None

    def get_hyperparameters(self, h, w, intrinsic, near_depth, far_depth):
        return frustum_geometry(self.opt, h, w, intrinsic, near_depth, far_depth)

    def stats(self) -> dict:
        """pnr_pquery_stats of the last call (a host read)."""
        if self._stats_dev is None:
            raise L.PnrError("perspective querier: no query yet")
        return dict(zip(L.PQUERY_STATS, self._stats_dev.tolist()))

    def query_points(self, pixel_idx_tensor, point_xyz_pers_tensor, point_xyz_w_tensor, actual_numpoints_tensor,
                     h, w, intrinsic, near_depth, far_depth, ray_dirs_tensor, cam_pos_tensor, cam_rot_tensor):
        """query_point_indices.py:78-102.  Returns (sample_pidx [1,R',SR,K] int32,
        sample_loc [1,R',SR,3], sample_loc_w, sample_ray_dirs, ray_mask [1,R] int8,
        vsize, ranges); rays are compacted by ray_mask only (a kept ray may have
        no neighbour).  B must be 1."""
        L.require_gpu(point_xyz_pers_tensor)
        opt = self.opt
        jitter = check_supported(opt)
        if point_xyz_pers_tensor.dim() == 3 and point_xyz_pers_tensor.shape[0] != 1:
            raise L.PnrError("batch size B > 1 is not supported (the reference uses B = 1)")
        for name, v in (("pixel_idx", pixel_idx_tensor), ("h", h), ("w", w), ("intrinsic", intrinsic)):
            if v is None:
                raise L.PnrError(f"perspective query (wcoord_query 0) needs {name}")
        dev = point_xyz_pers_tensor.device
        intr = intrinsic.detach().cpu().numpy() if torch.is_tensor(intrinsic) else np.asarray(intrinsic)
        h, w = L.host_scalar(h, int), L.host_scalar(w, int)
        geo = frustum_geometry(opt, h, w, intr.reshape(-1, 3, 3)[0], near_depth, far_depth)
        qp = pquery_params(opt, geo)
        pers = point_xyz_pers_tensor.detach().reshape(-1, 3).float().contiguous()
        pix = pixel_idx_tensor.to(dev).reshape(-1, 2).to(torch.int32).contiguous()
        N, R, SR, K = pers.shape[0], pix.shape[0], int(opt.SR), int(opt.K)
        if actual_numpoints_tensor is not None:
            N = min(N, int(actual_numpoints_tensor.reshape(-1)[0]))
        i32 = dict(dtype=torch.int32, device=dev)
        rows_pidx = torch.empty((max(R, 1), SR, K), **i32)
        rows_loc = torch.empty((max(R, 1), SR, 3), dtype=torch.float32, device=dev)
        rows_z = torch.empty((max(R, 1), SR), **i32)
        ray_mask = torch.zeros((1, R), dtype=torch.int8, device=dev)
        counts = torch.zeros(4, **i32)
        stats = torch.zeros(8, **i32)
        dims = (L.c_int32 * 3)(*[int(v) for v in geo.dims])
        scr = L.scratch("pnr_pquery_scratch_bytes", N, R, SR, dims, device=dev)
        st = L.stream_ptr(dev)
        L.check(L.lib().pnr_pquery(L.ctypes.byref(qp), L.ptr(pers), N, L.ptr(pix), R, L.ptr(rows_pidx), L.ptr(rows_loc),
                                   L.ptr(rows_z), L.ptr(ray_mask), L.ptr(counts), L.ptr(stats), L.ptr(scr), scr.numel(),
                                   st), "pnr_pquery")
        Rv = int(counts[0].item())   # the call's one host read
        sample_pidx = torch.empty((1, Rv, SR, K), **i32)
        sample_loc = torch.empty((1, Rv, SR, 3), dtype=torch.float32, device=dev)
        L.check(L.lib().pnr_pquery_compact(L.ptr(rows_pidx), L.ptr(rows_loc), R, SR, K, Rv, L.ptr(sample_pidx),
                                           L.ptr(sample_loc), st), "pnr_pquery_compact")
        self.last_slot_z = rows_z[:Rv].clone()
        self._stats_dev = stats
        self.count += 1
        if getattr(opt, "is_train", 0):
            sample_loc = getattr(self, jitter)(sample_loc, geo.vsize)
        sample_loc_w, sample_ray_dirs = self.pers2w(sample_loc, cam_rot_tensor, cam_pos_tensor)
        return sample_pidx, sample_loc, sample_loc_w, sample_ray_dirs, ray_mask, geo.vsize, geo.ranges

    def pers2w(self, point_xyz_pers, camrotc2w, campos):
        """query_point_indices.py:104-116."""
        z = point_xyz_pers[..., 2]
        xyz_c = torch.stack([point_xyz_pers[..., 0] * z, point_xyz_pers[..., 1] * z, z], dim=-1)
        xyz_w_shift = torch.sum(xyz_c[..., None, :] * camrotc2w.reshape(-1, 3, 3).float(), dim=-1)
        ray_dirs = xyz_w_shift / (torch.linalg.norm(xyz_w_shift, dim=-1, keepdims=True) + 1e-7)
        return xyz_w_shift + campos.reshape(-1, 3).float()[:, None, :], ray_dirs

    # The sample-depth jitters of a training query (opt.shpnt_jitter names one): the
    # centre's z moves inside its own depth voxel, torch's generator on the device.
    def passfunc(self, sample_loc, vsize):
        return sample_loc

    def uniform(self, sample_loc, vsize):
        """z += U(-1/2, 1/2) * vsize[2]."""
        u = torch.rand(sample_loc.shape[:-1], dtype=torch.float32, device=sample_loc.device)
        sample_loc[..., 2] += (u - 0.5) * float(vsize[2])
        return sample_loc

    def gaussian(self, sample_loc, vsize):
        """z += N(0, vsize[2] / 4) clamped to half a voxel."""
        half = float(vsize[2]) / 2
        n = torch.randn(sample_loc.shape[:-1], dtype=torch.float32, device=sample_loc.device) * (half / 2)
        sample_loc[..., 2] += n.clamp_(-half, half)
        return sample_loc
