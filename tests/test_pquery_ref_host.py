"""tests/pquery_ref.py -- the restatement the perspective-query kernels are
checked against bit for bit (test_gpu_pquery.py) -- pinned against independent
brute force, and the library's new boundary.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import pquery_ref as PR
from pquery_scene import popt, pscene

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _query(sc, **kw):
    return PR.query(sc["opt"], sc["pers"], sc["pixel_idx"], sc["H"], sc["W"], sc["intrinsic"], sc["near"], sc["far"],
                    **kw)


@pytest.fixture(scope="module")
def base():
    sc = pscene()
    return sc, _query(sc)


def test_geometry_hand_computed():
    """w != h, principal point off centre, powers of two so every quotient is
    exact: fx 64, fy 32, cx 24, cy 8, w 48, h 16, near 2, far 6, z_depth_dim 64,
    vscale (3, 2, 4)."""
    opt = popt(vscale=[3, 2, 4], z_depth_dim=64, radius_limit_scale=4.0, depth_limit_scale=2.0)
    K = np.array([[64, 0, 24], [0, 32, 8], [0, 0, 1]], F32)
    for fn in (PR.geometry, None):
        if fn is None:
            from pointnerf_amd.querier_p import frustum_geometry as fn
        g = fn(opt, 16, 48, K, 2.0, 6.0)
        assert np.array_equal(g.ranges, np.array([-0.375, -0.25, 2, 0.375, 0.25, 6], F32))
        assert g.ranges.dtype == F32
        assert np.array_equal(g.vdim, [48, 16, 64])
        assert np.array_equal(g.vsize, np.array([0.75 / 48, 0.5 / 16, 4 / 64], F32))
        assert np.array_equal(g.dims, [16, 8, 16])
        svs = g.svs if hasattr(g, "svs") else g.scaled_vsize
        rvs = g.rvs if hasattr(g, "rvs") else g.ray_vsize
        assert np.array_equal(svs, np.array([3 * 0.75 / 48, 2 * 0.5 / 16, 4 * 4 / 64], F32)) and svs.dtype == F32
        assert np.array_equal(rvs, g.vsize)
        assert g.radius_limit == F32(4 * 0.5 / 16) and g.depth_limit == F32(2 * 4 / 64)
    opt.vscale = [5, 3, 7]   # ceil dims
    assert np.array_equal(PR.geometry(opt, 16, 48, K, 2.0, 6.0).dims, [10, 6, 10])


def test_package_geometry_equals_restatement():
    from pointnerf_amd.querier_p import frustum_geometry
    sc = pscene(W=41, H=33, vscale=[3, 2, 2], cx=19.25, cy=17.5, radius_limit_scale=4.0, depth_limit_scale=2.0)
    a = PR.geometry(sc["opt"], 33, 41, sc["intrinsic"], 2.0, 6.0)
    b = frustum_geometry(sc["opt"], 33, 41, sc["intrinsic"], 2.0, 6.0)
    for x, y in ((a.ranges, b.ranges), (a.vsize, b.vsize), (a.dims, b.dims), (a.svs, b.scaled_vsize),
                 (a.rvs, b.ray_vsize), (a.radius_limit, b.radius_limit), (a.depth_limit, b.depth_limit)):
        assert np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype


@pytest.mark.parametrize("qs", [[3, 3, 3], [4, 2, 1], [1, 5, 2]])
def test_occupancy_is_union_of_query_blocks(qs):
    sc = pscene(1500)
    geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
    held, occ, _, inside, _ = PR.occupancy(geo, sc["pers"], qs)
    # independent: every cell asks whether a floor-binned point lies in [t - (q+1)/2 + 1, t + q/2]
    c = np.floor((sc["pers"] - geo.shift) / geo.svs).astype(np.int64)
    ok = np.all((c >= 0) & (c < geo.dims), 1)
    assert np.array_equal(ok, inside) and ok.sum() > 1000
    want = np.zeros(tuple(geo.dims), bool)
    for p in c[ok]:
        lo = [max(0, p[k] - qs[k] // 2) for k in range(3)]
        hi = [min(geo.dims[k], p[k] + (qs[k] + 1) // 2) for k in range(3)]
        want[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    assert np.array_equal(occ, want)
    assert held.sum() == len(np.unique(c[ok], axis=0)) and not (held & ~occ).any()


def test_selection_first_sr_set_bits_and_ray_mask(base):
    sc, q = base
    occ, geo = q["occ"], q["geo"]
    assert occ.sum(-1).max() > sc["opt"].SR          # SR 24 cuts columns short
    hit = np.nonzero(q["ray_mask"])[0]
    assert 0 < len(hit) < len(q["ray_mask"])
    for row, r in enumerate(hit):
        px, py = sc["pixel_idx"][r]
        ids = np.nonzero(occ[px // 2, py // 2])[0][:sc["opt"].SR]
        assert np.array_equal(q["slot_z"][row, :len(ids)], ids) and (q["slot_z"][row, len(ids):] == -1).all()
    for r in range(len(q["ray_mask"])):
        px, py = sc["pixel_idx"][r]
        ids = np.nonzero(occ[px // 2, py // 2])[0]
        assert q["ray_mask"][r] == (len(ids) > 0 and ids.max() > 0)


def test_column_holding_only_depth_id_0_is_a_miss():
    """A hand-placed point in depth voxel 0 with query_size z = 1: its column's
    only occupied id is 0, far_id > 0 fails, the ray is a miss."""
    sc = pscene(0, query_size=[1, 1, 1], kernel_size=[1, 1, 1])
    geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
    p0 = geo.shift + geo.svs * np.array([5.5, 7.5, 0.5], F32)    # voxel (5, 7, 0)
    p1 = geo.shift + geo.svs * np.array([9.5, 3.5, 1.5], F32)    # voxel (9, 3, 1)
    sc["pers"] = np.stack([p0, p1]).astype(F32)
    q = _query(sc)
    assert q["occ"][5, 7].sum() == 1 and q["occ"][5, 7, 0]
    mask = q["ray_mask"].reshape(sc["H"], sc["W"])
    assert mask[14:16, 10:12].sum() == 0                          # column (5, 7): rows 14-15, columns 10-11
    assert mask[6:8, 18:20].all() and mask.sum() == 4             # column (9, 3)
    assert (q["slot_z"][:, 0] == 1).all() and (q["sample_pidx"][:, 0, 0] == 1).all()


def _brute(sc, q, row, s, r):
    """Sorted xyz2 of the K nearest accepted points of one sample, from the
    points themselves: truncation cell inside the walk window, held voxel."""
    opt, geo = sc["opt"], q["geo"]
    ks = [int(v) for v in opt.kernel_size]
    px, py = (int(v) for v in sc["pixel_idx"][r])
    fx, fy, fz = px // int(geo.vscale[0]), py // int(geo.vscale[1]), int(q["slot_z"][row, s])
    t = ((sc["pers"] - geo.shift).astype(F32) / geo.svs).astype(F32)
    c = np.trunc(t).astype(np.int64)
    hx = (ks[0] + 1) // 2 - 1
    hz = min(hx, (ks[2] + 1) // 2 - 1)
    d = c - np.array([fx, fy, fz])
    win = (np.abs(d[:, 0]) <= hx) & (np.abs(d[:, 1]) <= hx) & (np.abs(d[:, 2]) <= hz)
    win &= np.all((t > -1) & (c < geo.dims), 1)
    # (the layers' rings and caps tile exactly this box: test_walk_window_matches_layered_order)
    ids = np.nonzero(win)[0]
    ids = np.array([i for i in ids if q["held"][tuple(c[i])]], np.int64)
    if not len(ids):
        return np.zeros(0, F32)
    centre = PR.centre(geo, px, py, fz)
    xy2, z2, xyz2 = PR.distances(sc["pers"], ids, centre, int(opt.NN))
    acc = ((geo.radius_limit2 == 0) | (xy2 <= geo.radius_limit2)) & ((geo.depth_limit2 == 0) | (z2 <= geo.depth_limit2))
    return np.sort(xyz2[acc])[:int(opt.K)]


@pytest.mark.parametrize("NN", [1, 2])
@pytest.mark.parametrize("limits", [(0.0, 0.0), (4.0, 2.0)])
def test_knn_equals_brute_force(NN, limits):
    sc = pscene(NN=NN, radius_limit_scale=limits[0], depth_limit_scale=limits[1], K=4)
    q = _query(sc)
    hit = np.nonzero(q["ray_mask"])[0]
    rng = np.random.default_rng(NN)
    checked = full = 0
    for row in rng.choice(len(hit), 60, replace=False):
        for s in np.nonzero(q["slot_z"][row] >= 0)[0][::5]:
            want = _brute(sc, q, row, s, hit[row])
            got = q["sample_pidx"][row, s]
            got = got[got >= 0]
            c = PR.centre(q["geo"], *(int(v) for v in sc["pixel_idx"][hit[row]]), int(q["slot_z"][row, s]))
            d = np.sort(PR.distances(sc["pers"], got.astype(np.int64), c, NN)[2]) if len(got) else np.zeros(0, F32)
            assert np.array_equal(d, want), (row, s)
            checked += 1
            full += len(got) == 4
    assert checked >= 100 and full >= 15      # enough samples whose K slots all filled (the replace phase ran)


def test_walk_window_matches_layered_order():
    """walk_cells visits each voxel of the window once; kernel (3,3,3) is the
    centre, then the 26 others; kernel (7,7,1) never leaves the sample's depth."""
    geo = PR.geometry(popt(), 32, 40, pscene(0)["intrinsic"], 2.0, 6.0)
    cells = PR.walk_cells(geo, [3, 3, 3], 5, 5, 5)
    assert cells[0] == (5, 5, 5) and len(cells) == 27 and len(set(cells)) == 27
    assert cells[1] == (4, 4, 4) and cells[-1] == (6, 6, 6)
    flat = PR.walk_cells(geo, [7, 7, 1], 5, 5, 5)
    assert len(flat) == 49 and all(c[2] == 5 for c in flat)
    assert len(PR.walk_cells(geo, [3, 3, 3], 0, 0, 0)) == 8          # clipped at the grid's corner
    tall = PR.walk_cells(geo, [5, 5, 3], 5, 5, 5)                    # zl = min(1, layer)
    assert len(tall) == len(set(tall)) == 25 * 3


def test_truncation_lists_a_point_occupancy_never_saw():
    """A point at shift_x - 0.3 svs_x: floor gives x = -1 (no occupancy), the
    insertion's truncation gives x = 0.  A second point holds voxel (0, y, z),
    so the sample there exists and finds both."""
    sc = pscene(0, K=4)
    geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
    inside = geo.shift + geo.svs * np.array([0.5, 6.5, 40.5], F32)
    ghost = inside.copy()
    ghost[0] = geo.shift[0] - F32(0.3) * geo.svs[0]
    sc["pers"] = np.stack([inside, ghost]).astype(F32)
    q = _query(sc)
    assert q["stats"]["n_points_in_grid"] == 1 and q["stats"]["n_voxels_held"] == 1
    alone = _query(dict(sc, pers=sc["pers"][1:]))
    assert alone["occ"].sum() == 0 and alone["ray_mask"].sum() == 0 and not alone["lists"]
    assert q["lists"][(0, 6, 40)] == [0, 1]
    hit = np.nonzero(q["ray_mask"])[0]
    row = list(sc["pixel_idx"][hit].tolist()).index([0, 12])
    s = list(q["slot_z"][row]).index(40)
    assert sorted(q["sample_pidx"][row, s].tolist()) == [-1, -1, 0, 1]


def test_p_overflow_keeps_seeded_subsets():
    sc = pscene(P=4)
    kept = []
    for seed in (0, 7):
        sc["opt"].grid_seed = seed
        geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
        held = PR.occupancy(geo, sc["pers"], [3, 3, 3])[0]
        lists, max_pts, over, c, inside = PR.insertion(geo, sc["pers"], held, 4, seed)
        assert max_pts == 11 and over > 20
        n = 0
        for cell, ids in lists.items():
            mem = [i for i in np.nonzero(np.all(c == cell, 1) & inside)[0]]
            if len(mem) > 4:
                want = sorted(sorted(mem, key=lambda i: (PR.hash32((seed + PR.SALT) & ((1 << 64) - 1), int(i)) << 32)
                                     | int(i))[:4])
                assert ids == want
                n += 1
            else:
                assert ids == mem
        assert n == over
        kept.append({k: tuple(v) for k, v in lists.items()})
    assert kept[0] != kept[1]


def test_restatement_refuses_undefined_ground():
    sc = pscene(500, kernel_size=[5, 5, 3], query_size=[3, 3, 3])
    with pytest.raises(PR.PQueryUndefined, match="wider"):
        _query(sc)
    sc = pscene(500, kernel_size=[3, 3, 3], query_size=[3, 3, 1])
    with pytest.raises(PR.PQueryUndefined, match="wider"):
        _query(sc)
    _query(pscene(200, kernel_size=[7, 7, 1], query_size=[7, 7, 1]))
    sc = pscene(0, z_depth_dim=400)
    geo = PR.geometry(sc["opt"], sc["H"], sc["W"], sc["intrinsic"], 2.0, 6.0)
    z = geo.shift[2] + geo.svs[2] * (np.arange(130, dtype=F32) * 2 + F32(0.5))
    sc["pers"] = np.stack([np.full(130, geo.shift[0] + geo.svs[0] * F32(3.5), F32),
                           np.full(130, geo.shift[1] + geo.svs[1] * F32(3.5), F32), z], -1).astype(F32)
    with pytest.raises(PR.PQueryUndefined, match="int8"):
        _query(sc)
    with pytest.raises(PR.PQueryUndefined):
        _query(pscene(100, NN=0))


def test_bad_pixels_and_points_are_counted_not_read(base):
    sc, q0 = base
    pers = np.concatenate([sc["pers"], np.array([[np.nan, 0, 3]], F32)])
    pix = np.concatenate([sc["pixel_idx"], np.array([[sc["W"], 0], [-1, 3]], np.int32)])
    q = _query(dict(sc, pers=pers, pixel_idx=pix))
    assert q["stats"]["n_bad_points"] == 1 and q["stats"]["n_bad_pixels"] == 2
    assert np.array_equal(q["ray_mask"][:-2], q0["ray_mask"]) and not q["ray_mask"][-2:].any()
    assert np.array_equal(q["sample_pidx"], q0["sample_pidx"])


def test_library_declares_and_exports_pquery():
    from pointnerf_amd import _lib as L
    for name in ("pnr_pquery", "pnr_pquery_compact", "pnr_pquery_scratch_bytes"):
        assert name in L.SIGNATURES
    assert L.ABI_VERSION >= 29
    lib = os.path.join(ROOT, "pointnerf_amd", "libpnr.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "pointnerf_amd/libpnr.so"])
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert {"pnr_pquery", "pnr_pquery_compact", "pnr_pquery_scratch_bytes"} <= set(re.findall(r" T (pnr_[a-z0-9_]+)", out))
    # validation runs on the host and never throws across the ABI
    h = L.lib()
    assert h.pnr_pquery(None, None, 0, None, 0, None, None, None, None, None, None, None, 0, None) == L.PNR_EINVAL
    q = L.PQueryParams()
    q.scaled_vsize[:] = q.ray_vsize[:] = [0.1, 0.1, 0.1]
    q.dims[:] = [4, 4, 4]
    q.vscale[:] = [1, 1, 1]
    q.w = q.h = 4
    q.SR, q.K, q.P, q.NN = 4, 8, 4, 2
    q.kernel_size[:] = [5, 5, 3]
    q.query_size[:] = [3, 3, 3]
    fake = L.c_void_p(0x1000)     # never dereferenced: the check runs first
    rc = h.pnr_pquery(L.ctypes.byref(q), fake, 1, fake, 1, fake, fake, fake, fake, fake, fake, fake, 1 << 30, None)
    assert rc == L.PNR_EINVAL and b"wider than query_size" in h.pnr_last_error()
    q.kernel_size[:] = [3, 3, 3]
    q.NN = 0
    rc = h.pnr_pquery(L.ctypes.byref(q), fake, 1, fake, 1, fake, fake, fake, fake, fake, fake, fake, 1 << 30, None)
    assert rc == L.PNR_EINVAL and b"NN" in h.pnr_last_error()
