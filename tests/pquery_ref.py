"""Serial numpy restatement of the perspective-frustum point query
(models/neural_points/query_point_indices.py, --wcoord_query 0):
geometry, occupancy, column selection, insertion with its truncation, the
layered walk, compaction and pers2w.  fp32 wherever the reference computes in
fp32, one rounding per operation and no fused multiply-add; the sample centres
go through fp64 where the reference's `+ 0.5` literals promote them.

It raises PQueryUndefined when an input leaves the range in which the reference
itself is defined (its int8 slot ranks, a kernel wider than the query block),
so no test can pass on undefined ground.  Pixels outside the frame and
non-finite points are handled as pnr_pquery documents them (misses / dropped,
counted).  A voxel listing more than P points keeps the P of smallest
res_hash32(grid_seed + salt, id), in ascending id (the world grid's rule)."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
SALT = 0x632BE59BD9B4E019
_M64 = (1 << 64) - 1


class PQueryUndefined(ValueError):
    pass


def hash32(seed, i):
    """res_hash32 (pnr_common.h) in Python integers."""
    z = (seed ^ (i * 0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z >> 32


def geometry(opt, h, w, intrinsic, near, far):
    """get_hyperparameters (:52-75) with an fp32 intrinsic and fp32 near / far,
    as NeuralPoints.forward hands them over."""
    if getattr(opt, "inverse", 0):
        raise PQueryUndefined("inverse 1 is not restated")
    K = np.asarray(intrinsic, F32).reshape(3, 3)
    h, w = int(h), int(w)
    near, far = F32(near), F32(far)
    x_rl, x_rh = -K[0, 2] / K[0, 0], (F32(w) - K[0, 2]) / K[0, 0]          # fp32
    y_rl, y_rh = -K[1, 2] / K[1, 1], (F32(h) - K[1, 2]) / K[1, 1]
    z_r = far - near
    ranges = np.array([x_rl, y_rl, near, x_rh, y_rh, far], dtype=F32)
    vdim = np.array([w, h, opt.z_depth_dim], dtype=np.int32)
    # fp32 / int32 promotes to fp64, the array is fp32
    vsize = np.array([np.float64(x_rh - x_rl) / vdim[0], np.float64(y_rh - y_rl) / vdim[1],
                      np.float64(z_r) / vdim[2]], dtype=F32)
    vscale = np.array(opt.vscale, dtype=np.int32)
    dims = np.ceil(vdim / vscale).astype(np.int32)
    svs = (vsize.astype(np.float64) * vscale).astype(F32)
    rvs = (svs.astype(np.float64) / vscale).astype(F32)
    radius_limit = F32(F32(opt.radius_limit_scale) * max(vsize[0], vsize[1]))
    depth_limit = F32(F32(opt.depth_limit_scale) * vsize[2])
    return SimpleNamespace(ranges=ranges, vsize=vsize, vdim=vdim, vscale=vscale, dims=dims, svs=svs, rvs=rvs,
                           shift=ranges[:3].copy(), radius_limit=radius_limit, depth_limit=depth_limit,
                           radius_limit2=F32(radius_limit * radius_limit), depth_limit2=F32(depth_limit * depth_limit),
                           w=w, h=h)


def _sizes(opt):
    ks = [int(v) for v in opt.kernel_size]
    qs = [int(v) for v in getattr(opt, "query_size", (0, 0, 0))]
    if qs[0] == 0:
        qs = list(ks)
    return ks, qs


def check_defined(opt):
    ks, qs = _sizes(opt)
    hx = (ks[0] + 1) // 2 - 1
    hz = min(hx, (ks[2] + 1) // 2 - 1)
    if hx > (qs[0] + 1) // 2 - 1 or hx > (qs[1] + 1) // 2 - 1 or hz > (qs[2] + 1) // 2 - 1:
        raise PQueryUndefined(f"kernel_size {ks} is wider than query_size {qs}")
    if opt.NN < 1:
        raise PQueryUndefined("NN = 0 draws from time()")


def quotients(geo, pers):
    """(p - shift) / scaled_vsize in fp32, [N,3], and the rows that are finite."""
    p = np.asarray(pers, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = ((p - geo.shift).astype(F32) / geo.svs).astype(F32)
    ok = np.isfinite(p).all(1) & np.isfinite(t).all(1)
    return t, ok


def occupancy(geo, pers, query_size):
    """get_occ_vox (:265-314): held [dims] (voxels a floor-binned point lies in),
    occ [dims] (their query_size blocks), the floor cells [N,3] and in-grid flags."""
    t, ok = quotients(geo, pers)
    dims = geo.dims.astype(np.int64)
    with np.errstate(all="ignore"):
        c = np.floor(np.where(ok[:, None], t, -1)).astype(np.int64)
    inside = ok & np.all((c >= 0) & (c < dims), 1)
    held = np.zeros(tuple(dims), bool)
    occ = np.zeros(tuple(dims), bool)
    q = [int(v) for v in query_size]
    for cx, cy, cz in np.unique(c[inside], axis=0):
        held[cx, cy, cz] = True
        occ[max(0, cx - q[0] // 2):cx + (q[0] + 1) // 2, max(0, cy - q[1] // 2):cy + (q[1] + 1) // 2,
            max(0, cz - q[2] // 2):cz + (q[2] + 1) // 2] = True
    return held, occ, c, inside, ok


def insertion(geo, pers, held, P, seed):
    """insert_vox_points (:368-413) on the serial schedule: {cell: ids} of the
    held voxels, by the quotient truncated toward zero; plus (max points per
    voxel, voxels over P)."""
    t, ok = quotients(geo, pers)
    dims = geo.dims.astype(np.int64)
    with np.errstate(all="ignore"):
        c = np.trunc(np.where(ok[:, None], t, -9)).astype(np.int64)       # C's float -> int conversion
    inside = ok & np.all((c >= 0) & (c < dims), 1)
    lists = {}
    for i in np.nonzero(inside)[0]:
        key = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
        if held[key]:
            lists.setdefault(key, []).append(int(i))
    max_pts, over = 0, 0
    for key, ids in lists.items():
        max_pts = max(max_pts, len(ids))
        if len(ids) > P:
            over += 1
            lists[key] = sorted(sorted(ids, key=lambda i: (hash32((seed + SALT) & _M64, i) << 32) | i)[:P])
    return lists, max_pts, over, c, inside


def centre(geo, px, py, fz):
    """The sample centre (:534-536): float + int * float in fp32, the 0.5 terms in fp64."""
    fx, fy = px // int(geo.vscale[0]), py // int(geo.vscale[1])
    cx = F32(np.float64(F32(geo.shift[0] + F32(F32(fx) * geo.svs[0])))
             + (px % int(geo.vscale[0]) + 0.5) * np.float64(geo.rvs[0]))
    cy = F32(np.float64(F32(geo.shift[1] + F32(F32(fy) * geo.svs[1])))
             + (py % int(geo.vscale[1]) + 0.5) * np.float64(geo.rvs[1]))
    cz = F32(np.float64(geo.shift[2]) + (fz + 0.5) * np.float64(geo.svs[2]))
    return cx, cy, cz


def walk_cells(geo, ks, fx, fy, fz):
    """The voxels query_neigh_along_ray_layered visits (:549-561), in its order."""
    dims = [int(v) for v in geo.dims]
    out = []
    for layer in range((ks[0] + 1) // 2):
        zl = min((ks[2] + 1) // 2 - 1, layer)
        for x in range(max(-fx, -layer), min(dims[0] - fx, layer + 1)):
            for y in range(max(-fy, -layer), min(dims[1] - fy, layer + 1)):
                for z in range(max(-fz, -zl), min(dims[2] - fz, zl + 1)):
                    if max(abs(x), abs(y)) != layer and (abs(z) != zl if zl == layer else True):
                        continue
                    out.append((fx + x, fy + y, fz + z))
    return out


def distances(pers, ids, c, NN):
    """(xy2, z2, xyz2) of the points ids to the centre c, fp32 (:568-572)."""
    p = pers[ids]
    cx, cy, cz = c
    if NN < 2:
        xv, yv = (p[:, 0] - cx).astype(F32), (p[:, 1] - cy).astype(F32)
    else:
        xv = ((p[:, 0] * p[:, 2]).astype(F32) - F32(cx * cz)).astype(F32)
        yv = ((p[:, 1] * p[:, 2]).astype(F32) - F32(cy * cz)).astype(F32)
    xy2 = ((xv * xv).astype(F32) + (yv * yv).astype(F32)).astype(F32)
    zv = (p[:, 2] - cz).astype(F32)
    z2 = (zv * zv).astype(F32)
    return xy2, z2, (xy2 + z2).astype(F32)


def knn(pers, lists, cells, c, K, NN, r2, d2):
    """The K slots of one sample (:566-594): fill in visit order, then replace
    the first farthest when strictly closer."""
    ids = [i for cell in cells for i in lists.get(cell, ())]
    out = np.full(K, -1, np.int32)
    if not ids:
        return out
    ids = np.asarray(ids, np.int64)
    xy2, z2, xyz2 = distances(pers, ids, c, NN)
    acc = ((r2 == 0) | (xy2 <= r2)) & ((d2 == 0) | (z2 <= d2))
    buf, kid, far2, far_ind = [0.0] * K, 0, 0.0, 0
    for i, d in zip(ids[acc].tolist(), xyz2[acc].tolist()):      # fp32 values held exactly in Python floats
        if kid < K:
            out[kid], buf[kid] = i, d
            if d > far2:
                far2, far_ind = d, kid
            kid += 1
        elif d < far2:
            out[far_ind], buf[far_ind] = i, d
            far2 = d
            for j in range(K):
                if buf[j] > far2:
                    far2, far_ind = buf[j], j
    return out


def pers2w(sample_loc, camrot, campos):
    """pers2w (:104-116) in fp32: (sample_loc_w, sample_ray_dirs)."""
    s = np.asarray(sample_loc, F32)
    R = np.asarray(camrot, F32).reshape(3, 3)
    xc = np.stack([(s[..., 0] * s[..., 2]).astype(F32), (s[..., 1] * s[..., 2]).astype(F32), s[..., 2]], -1)
    sh = (xc[..., None, :] * R).astype(F32).sum(-1, dtype=F32)
    n = np.sqrt((sh * sh).astype(F32).sum(-1, keepdims=True, dtype=F32)).astype(F32)
    dirs = (sh / (n + F32(1e-7))).astype(F32)
    return (sh + np.asarray(campos, F32).reshape(3)).astype(F32), dirs


def query(opt, pers, pixel_idx, h, w, intrinsic, near, far, camrot=None, campos=None):
    """query_points (:78-102) for B = 1 without the training jitter.  pers [N,3]
    perspective coordinates, pixel_idx [R,2] (column, row).  Returns a dict:
    sample_pidx [R',SR,K], sample_loc [R',SR,3], slot_z [R',SR], ray_mask [R],
    stats, lists, held, occ, geo (and sample_loc_w / sample_ray_dirs with a camera)."""
    check_defined(opt)
    ks, qs = _sizes(opt)
    geo = geometry(opt, h, w, intrinsic, near, far)
    pers = np.ascontiguousarray(np.asarray(pers, F32).reshape(-1, 3))
    pix = np.asarray(pixel_idx).reshape(-1, 2).astype(np.int64)
    SR, K, P = int(opt.SR), int(opt.K), int(opt.P)
    seed = int(getattr(opt, "grid_seed", 0))
    held, occ, _, inside, ok = occupancy(geo, pers, qs)
    per_col = held.sum(-1)
    limit = min(127, int(opt.max_o)) if getattr(opt, "max_o", None) else 127
    if per_col.size and int(per_col.max()) > limit:
        raise PQueryUndefined(f"{int(per_col.max())} held voxels in one column: the reference's int8 slot ranks "
                              f"hold {limit}")
    lists, max_pts, over, _, _ = insertion(geo, pers, held, P, seed)
    good = (pix[:, 0] >= 0) & (pix[:, 0] < geo.w) & (pix[:, 1] >= 0) & (pix[:, 1] < geo.h)
    R = pix.shape[0]
    ray_mask = np.zeros(R, np.int8)
    col_ids = {}
    for r in np.nonzero(good)[0]:
        col = (int(pix[r, 0]) // int(geo.vscale[0]), int(pix[r, 1]) // int(geo.vscale[1]))
        if col not in col_ids:
            col_ids[col] = np.nonzero(occ[col])[0]
        z = col_ids[col]
        ray_mask[r] = 1 if (len(z) and z[-1] > 0) else 0          # far_id > 0
    hit = np.nonzero(ray_mask)[0]
    sample_pidx = np.full((len(hit), SR, K), -1, np.int32)
    sample_loc = np.zeros((len(hit), SR, 3), F32)
    slot_z = np.full((len(hit), SR), -1, np.int32)
    r2, d2 = geo.radius_limit2, geo.depth_limit2
    for row, r in enumerate(hit):
        px, py = int(pix[r, 0]), int(pix[r, 1])
        fx, fy = px // int(geo.vscale[0]), py // int(geo.vscale[1])
        z = col_ids[(fx, fy)][:SR]
        slot_z[row, :len(z)] = z
        for s in range(SR):
            fz = int(slot_z[row, s])
            c = centre(geo, px, py, fz)
            sample_loc[row, s] = c
            if fz >= 0:
                sample_pidx[row, s] = knn(pers, lists, walk_cells(geo, ks, fx, fy, fz), c, K, int(opt.NN), r2, d2)
    stats = dict(n_points_in_grid=int(inside.sum()), n_voxels_held=int(held.sum()),
                 max_held_per_column=int(per_col.max()) if per_col.size else 0, max_points_per_voxel=max_pts,
                 n_voxels_over_p=over, n_bad_pixels=int((~good).sum()), n_bad_points=int((~ok).sum()))
    out = dict(sample_pidx=sample_pidx, sample_loc=sample_loc, slot_z=slot_z, ray_mask=ray_mask, stats=stats,
               lists=lists, held=held, occ=occ, geo=geo, vsize=geo.vsize, ranges=geo.ranges)
    if camrot is not None:
        out["sample_loc_w"], out["sample_ray_dirs"] = pers2w(sample_loc, camrot, campos)
    return out
