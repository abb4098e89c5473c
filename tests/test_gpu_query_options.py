"""World-grid build and query (grid.hip, query.hip behind
querier.lighting_fast_querier) bit for bit against the CPU oracle off the
shipped flag sets: the option matrix of tests/query_cases.py -- query sizes
1, 2, 4, 5, 7 and mixed (the dilation's loops and its unrolled forms, the
asymmetric even window), kernel sizes 1, 5, 7, 9 and mixed on the generic
layered walk at K 1 / 8 / 16 / 32 (k_knn<8|16|32, 0, .>), the radius test off
and tighter, anisotropic vsize / vscale, a cloud crossing ranges, flat clouds
(dims[2] = 2, 3, 6).  Every comparison is exact: integers and gathered or
recomputed fp32 values with the reference's operation order.

Besides the per-case comparison: the host-geometry build equals the device
one, one engine reused across builds of other sizes equals fresh engines, and
two runs are bitwise equal.

Found by this suite: no kernel bug -- all 25 cases equal the oracle, so no
option value is refused in place of a case.  One claim of the
table's author did not hold under the oracle: the flat clouds do overflow P
(13 points in a voxel of P = 9), so n_points_dropped is compared with the
oracle's count, which is 0 on every other case."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import query_cases as QC

pytestmark = pytest.mark.gpu


def _engine(opt, cuda):
    from pointnerf_amd.querier import lighting_fast_querier
    return lighting_fast_querier(cuda, opt)


def _dev(sc, cuda):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    return t(sc["xyz"]), t(sc["raydir"]), t(sc["campos"]), t(sc["camrot"])


def _unpack(bits, n):
    bits = bits.cpu().numpy().view(np.uint32)
    return ((bits[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:n].astype(np.uint8)


def _state(q, sc, cuda, opt=None):
    """q.opt = opt, one query of the scene on q: export(), the query's buffers, stats()."""
    opt = opt or sc["opt"]
    q.opt = opt
    xyz, rd, cp, cr = _dev(sc, cuda)
    bufs, hp, _, _ = q.run(xyz, rd, cp, cr, 2.0, 6.0)
    out = dict(q.grid.export())
    c = bufs.read_counts()
    S, R = c["S_filled"], rd.shape[0]
    out.update(counts=bufs.counts.clone(), n_filled=bufs.n_filled[:R].clone(), fill_rs=bufs.fill_rs[:S].clone(),
               pidx=bufs.pidx[: S * opt.K].clone(), sample_w=bufs.sample_w[: S * 3].clone(),
               sample_p=bufs.sample_p[: S * 3].clone(), valid_list=bufs.valid_list[: c["S_valid"]].clone(),
               shift=torch.from_numpy(np.asarray(hp["shift"])), dims=torch.from_numpy(np.asarray(hp["dims"])),
               ranges=torch.from_numpy(np.asarray(hp["ranges"])))
    # slot_d of the filled slots (the rest of a ray's row is never written)
    sd = bufs.slot_d[: R * opt.SR].view(R, opt.SR)
    keep = torch.arange(opt.SR, device=cuda)[None, :] < out["n_filled"][:, None]
    out["slot_d"] = sd[keep].clone()
    return out, q.grid.stats()


def _same_state(got, want, what):
    (g, gs), (w, ws) = got, want
    assert gs == ws, (what, gs, ws)
    assert g.keys() == w.keys()
    for k in w:
        assert torch.equal(g[k], w[k]), (what, k)


@pytest.mark.parametrize("name", list(QC.CASES))
def test_case_equals_oracle(cuda, name):
    sc, _, ref = QC.build(name)
    opt, g = sc["opt"], ref["grid"]
    q = _engine(opt, cuda)
    xyz, rd, cp, cr = _dev(sc, cuda)
    R, SR, K = rd.shape[0], opt.SR, opt.K

    # the build: geometry, tables, statistics
    hp = q.grid.build(opt, xyz)
    for k in ("shift", "dims", "vsize_s", "ranges"):
        assert np.array_equal(np.asarray(hp[k]), np.asarray(g["hp"][k])), k
    t = q.grid.export()
    assert np.array_equal(t["coor_2_occ"].cpu().numpy(), g["coor_2_occ"])
    assert np.array_equal(_unpack(t["occ_bits"], g["coor_occ"].size), g["coor_occ"])
    assert np.array_equal(t["occ_numpnts"].cpu().numpy(), g["occ_numpnts"])
    assert np.array_equal(t["occ_2_pnts"].cpu().numpy(), g["occ_2_pnts"])
    st = q.grid.stats()
    assert st["n_voxels"] == g["n_occ"] <= opt.max_o
    # no voxel overflows P -- but in the flat clouds, whose pressed columns reach 13 points of
    # P = 9: there the seeded reservoir runs (the tables above hold its subsets)
    dropped = int(np.maximum(g["occ_numpnts"][: g["n_occ"]] - opt.P, 0).sum())
    assert st["n_points_dropped"] == dropped and (dropped == 0) == (name not in QC.FLAT_DIMS_Z)
    assert st["dims"] == [int(d) for d in g["hp"]["dims"]] and st["device_geometry"]

    # the query's own buffers (same grid: the point tensor and the options are unchanged)
    bufs, _, _, _ = q.run(xyz, rd, cp, cr, 2.0, 6.0)
    c = bufs.read_counts()
    nf = bufs.n_filled[:R].cpu().numpy()
    assert np.array_equal(nf, ref["n_filled"])
    keep = np.arange(SR)[None, :] < nf[:, None]
    sd = bufs.slot_d[: R * SR].cpu().numpy().astype(np.int32).reshape(R, SR)
    assert np.array_equal(sd[keep], ref["slot_d"][keep])
    assert c["S_filled"] == nf.sum() and c["R_hit"] == (nf > 0).sum()
    assert c["R_valid"] == ref["ray_mask"].sum()
    assert c["n_pairs"] == (ref["pidx_dense"] >= 0).sum()
    assert c["S_valid"] == (ref["pidx_dense"] >= 0).any(-1).sum()
    assert np.array_equal(bufs.pidx[: c["S_filled"] * K].cpu().numpy().reshape(-1, K), ref["pidx_dense"][keep])

    # the reference-shaped outputs
    out = q.query_points(None, None, xyz[None], None, 800, 800, None, 2.0, 6.0, rd[None], cp[None], cr[None])
    pidx, loc, loc_w, dirs, ray_mask = [x.cpu().numpy() for x in out[:5]]
    assert np.array_equal(ray_mask[0], ref["ray_mask"])
    assert pidx.shape == (1,) + ref["sample_pidx"].shape and pidx.dtype == np.int32
    assert np.array_equal(pidx[0], ref["sample_pidx"])          # same neighbours, same order
    assert np.array_equal(loc_w[0], ref["sample_loc_w"])
    assert np.array_equal(loc[0], ref["sample_loc"])
    assert np.array_equal(dirs[0], ref["sample_ray_dirs"])
    np.testing.assert_array_equal(out[6], ref["ranges"])


@pytest.mark.parametrize("name", ["aniso", "aniso-k5-q542", "clipped", "flat-k5-K16"])
def test_host_geometry_build_equals_device_build(cuda, name):
    sc = QC.build(name)[0]
    opt_host = SimpleNamespace(**{**vars(sc["opt"]), "grid_host_bbox": True})
    dev = _state(_engine(sc["opt"], cuda), sc, cuda)
    host = _state(_engine(opt_host, cuda), sc, cuda, opt_host)
    assert dev[1].pop("device_geometry") and not host[1].pop("device_geometry")
    assert int(dev[0]["counts"][1]) > 300
    _same_state(host, dev, name)


def test_one_engine_reused_across_option_sets_equals_fresh_engines(cuda):
    """Four layers at K 32 on the largest tables, then kernel and query 1, the
    mixed query box, a grid three cells thin, and K 16 on a dense cloud: after
    each step the reused engine's tables, statistics and query buffers are a
    fresh engine's -- the coarse map, the dilation scratch and the buffers sized
    by K carry nothing over from a build with other sizes."""
    chain = ["k777-K32", "q111-k111", "q535", "flat-k3", "k555-K16"]
    reused = _engine(QC.build(chain[0])[0]["opt"], cuda)
    for name in chain:
        sc = QC.build(name)[0]
        got = _state(reused, sc, cuda)
        want = _state(_engine(sc["opt"], cuda), sc, cuda)
        assert int(want[0]["counts"][1]) > 150, name
        _same_state(got, want, name)


@pytest.mark.parametrize("name", ["k777-K32", "q535"])
def test_two_runs_bitwise_equal(cuda, name):
    sc = QC.build(name)[0]
    q = _engine(sc["opt"], cuda)
    a = _state(q, sc, cuda)
    q.grid.key = None   # force a rebuild
    b = _state(q, sc, cuda)
    _same_state(b, a, name)
