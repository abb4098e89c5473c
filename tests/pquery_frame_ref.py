"""TEST INFRASTRUCTURE ONLY -- the fused perspective frame restated
for its tests: the pnr_query_bufs that pnr_pquery_bufs must write, derived in
numpy from a perspective query's reference-shaped rows (tests/pquery_ref.query, or
pnr_pquery's own rows), and the perspective mode of the composite reference
(composite_ref, imported and not edited): the unfilled slots lie at z_unfilled
instead of the world origin's depth, and a ray is a hit when ray_hit says so.

The scenes and cases of tests/test_gpu_pquery_frame.py live here so that the CPU
test (tests/test_pquery_frame_host.py) checks the same inputs."""
from __future__ import annotations

import numpy as np
import torch

import composite_ref as CR
import pquery_ref as PR
from oracle import oracle as O
from oracle import oracle_grad as OG
from pquery_scene import pscene

F32 = np.float32

# ---------------------------------------------------------------------- scenes
SCENE_R = 1280
SCENE_HIT = dict(A=1012, B=976, C=976)   # hit rays (A: the base scene's 976 and the lone point's 36)


def scene(name):
    """A: the lone-point scene of test_gpu_pquery_render.py; B: 80 slots over 400
    depth ids (rays past slot 64); C: SR 8 (columns with more occupied ids than SR)."""
    if name == "A":
        from test_gpu_pquery_render import lone_point_scene
        return lone_point_scene()
    from test_gpu_pquery_render import features
    if name == "B":
        return features(pscene(SR=80, z_depth_dim=400, query_size=[3, 3, 9]))
    assert name == "C"
    return features(pscene(SR=8))


def subsets(R=SCENE_R):
    """Shuffled pixel subsets that are no multiple of 64 or 256: 1279 and 777 rows."""
    rng = np.random.default_rng(29)
    return [rng.permutation(R)[:n] for n in (1279, 777)]


def ref_query(sc, pix=None, pers=None):
    return PR.query(sc["opt"], sc["pers"] if pers is None else pers, sc["pixel_idx"] if pix is None else pix, sc["H"],
                    sc["W"], sc["intrinsic"], sc["near"], sc["far"], sc["camrot"], sc["campos"])


def z_unfilled(geo):
    """The centre depth of fz = -1, as PR.centre forms it."""
    return float(F32(np.float64(geo.shift[2]) - 0.5 * np.float64(geo.svs[2])))


# -------------------------------------------------------------- expected buffers
def expected_bufs(ray_mask, slot_z, sample_pidx, sample_loc, SR, K):
    """The pnr_query_bufs of a perspective query from its reference-shaped rows:
    ray_mask [R], and for the hit rays in ray order slot_z [R',SR], sample_pidx
    [R',SR,K], sample_loc [R',SR,3].  Returns numpy arrays by pnr_query_bufs' names
    (sized by their contents: S_filled rows) plus ray_hit and counts[0..4]."""
    ray_mask = np.asarray(ray_mask).reshape(-1)
    R = ray_mask.shape[0]
    hit = np.nonzero(ray_mask)[0]
    slot_z = np.asarray(slot_z).reshape(len(hit), SR)
    pid = np.asarray(sample_pidx).reshape(len(hit), SR, K)
    loc = np.asarray(sample_loc, F32).reshape(len(hit), SR, 3)
    filled = slot_z >= 0
    # the ids fill the first slots of a row
    assert all(f[:n].all() and not f[n:].any() for f, n in zip(filled, filled.sum(1)))
    n_filled = np.zeros(R, np.int32)
    n_filled[hit] = filled.sum(1)
    ray_off = np.concatenate([[0], np.cumsum(n_filled)]).astype(np.int32)
    rows, slots = np.nonzero(filled)                       # row-major: ray after ray, slot after slot
    fill_rs = (hit[rows] * SR + slots).astype(np.int32)
    pidx = pid[rows, slots].astype(np.int32)
    vflag = (pidx >= 0).any(1).astype(np.int32)
    valid_off = np.concatenate([[0], np.cumsum(vflag)]).astype(np.int32)
    ray_vcnt = np.zeros(R, np.int32)
    np.add.at(ray_vcnt, hit[rows], vflag)
    ray_row = np.concatenate([[0], np.cumsum(ray_vcnt > 0)]).astype(np.int32)
    counts = np.array([len(rows), vflag.sum(), len(hit), (ray_vcnt > 0).sum(), (pidx[vflag > 0] >= 0).sum()], np.int32)
    return dict(ray_hit=ray_mask.astype(np.int8), n_filled=n_filled, ray_off=ray_off, fill_rs=fill_rs,
                slot_d=slot_z[rows, slots].astype(np.uint16), pidx=pidx, sample_p=loc[rows, slots], vflag=vflag,
                valid_off=valid_off, valid_list=np.nonzero(vflag)[0].astype(np.int32), ray_vcnt=ray_vcnt,
                ray_row=ray_row, counts=counts)


def expected_from_query(q, SR, K):
    return expected_bufs(q["ray_mask"], q["slot_z"], q["sample_pidx"], q["sample_loc"], SR, K)


def check_invariants(e, R, SR, K):
    """What any such buffers satisfy, whatever the scene."""
    S = int(e["counts"][0])
    assert e["n_filled"].shape == (R,) and e["ray_off"].shape == (R + 1,) and e["ray_row"].shape == (R + 1,)
    assert ((e["n_filled"] >= 0) & (e["n_filled"] <= SR)).all()
    assert (e["n_filled"][e["ray_hit"] == 0] == 0).all()                  # a miss has no rows
    assert e["ray_off"][0] == 0 and np.array_equal(np.diff(e["ray_off"]), e["n_filled"]) and e["ray_off"][-1] == S
    r = np.repeat(np.arange(R), e["n_filled"])
    s = np.arange(S) - e["ray_off"][r]
    assert np.array_equal(e["fill_rs"], r * SR + s)
    assert e["pidx"].shape == (S, K) and e["sample_p"].shape == (S, 3) and e["slot_d"].shape == (S,)
    assert np.array_equal(e["vflag"], (e["pidx"] >= 0).any(1).astype(np.int32))
    assert e["valid_off"][0] == 0 and np.array_equal(np.diff(e["valid_off"]), e["vflag"])
    assert np.array_equal(e["valid_list"], np.nonzero(e["vflag"])[0])
    assert np.array_equal(e["ray_vcnt"], np.bincount(r, weights=e["vflag"], minlength=R).astype(np.int32))
    assert np.array_equal(np.diff(e["ray_row"]), (e["ray_vcnt"] > 0).astype(np.int32))
    assert list(e["counts"]) == [S, e["vflag"].sum(), (e["ray_hit"] != 0).sum(), (e["ray_vcnt"] > 0).sum(),
                                 (e["pidx"][e["vflag"] > 0] >= 0).sum()]
    # the depth ids of a ray ascend strictly
    for a, n in zip(e["ray_off"][:-1], e["n_filled"]):
        assert (np.diff(e["slot_d"][a:a + n].astype(np.int64)) > 0).all()


# ------------------------------------------------------------ composite reference
def perspective_case(b, seed):
    """ray_hit and the three z_unfilled of a composite_ref.make_bufs case: hit at
    random, with at least one hit ray that has no valid sample and one missed ray
    that has filled rows; z_unfilled below, inside and above the filled depths."""
    rng = np.random.default_rng(9000 + seed)
    R = b["R"]
    vc, nf = b["ray_vcnt"].numpy(), b["n_filled"].numpy()
    hit = (rng.random(R) < 0.7).astype(np.int8)
    empty = np.nonzero(vc == 0)[0]
    full = np.nonzero(nf > 0)[0]
    if len(empty):
        hit[empty[0]] = 1
    if len(full):
        hit[full[-1]] = 0
    z = b["sample_p"].numpy()[:, 2] if b["S"] else np.array([0.0], F32)
    zs = (float(F32(z.min() - 0.05)), float(F32(0.5 * (float(z.min()) + float(z.max())))), float(F32(z.max() + 0.05)))
    return torch.from_numpy(hit), zs


def scatter_dense_p(b, feat, zu, feat_rows=0):
    """composite_ref.scatter_dense with the unfilled slots at depth zu."""
    loc, rv, idx = CR.scatter_dense(b, feat, feat_rows)
    n = b["n_filled"].numpy()
    for r in range(b["R"]):
        loc[r, n[r]:, 2] = F32(zu)
    return loc, rv, idx


def composite_reference_p(b, feat, ray_hit, zu, params, dtype):
    """ray_color [R,C], opacity [R,SR], is_bg [R], ray_mask [R] int8 of
    pnr_composite_fwd_p on the buffers: composite_ref.composite_reference's forward
    with the hit mask and the unfilled depth of the perspective mode.  A hit ray
    without a valid sample marches like any other (opacity 0, colour bg bg_T)."""
    R, SR = b["R"], b["SR"]
    CF = feat.shape[1]
    loc, rv, (ri, si, rowi) = scatter_dense_p(b, feat, zu, params.get("feat_rows", 0))
    rdist = O.ray_dist(loc, rv, params["vsize_z"], params["unit"])   # fp32 numpy
    rows = torch.nan_to_num(feat, nan=0.0).to(dtype)
    dense = torch.zeros((R, SR, CF), dtype=dtype).index_put((ri, si), rows[rowi])
    bg = params.get("bg")
    bg_ = None if bg is None else bg.to(dtype)
    color, opacity, _, _, bgT = OG.ray_march_full(torch.from_numpy(rdist).to(dtype), torch.from_numpy(rv), dense, bg_)
    mask = ray_hit.bool()
    color, opacity, is_bg = color.detach().clone(), opacity.detach().clone(), bgT.detach()[:, 0].clone()
    color[~mask] = bg_ if bg_ is not None else 0.0
    opacity[~mask] = 0.0
    is_bg[~mask] = 1.0
    return dict(ray_color=color, opacity=opacity, is_bg=is_bg, ray_mask=mask.to(torch.int8), ray_dist=rdist)


# (SR, C, bg, unit): every SR and both C of the issue, bg and unit on and off
P_SR = (1, 2, 63, 64, 65, 80, 127, 128)
P_CASES = [(sr, c, bg, unit) for i, sr in enumerate(P_SR)
           for c, bg, unit in (((3, True, 1), (128, False, 0)) if i % 2 == 0 else ((3, False, 0), (128, True, 1)))]
P_CASES += [(128, 3, True, 0), (128, 128, False, 1), (65, 3, False, 1), (65, 128, True, 0)]
P_R = 48


def case_inputs(SR, C, bg, unit):
    """(bufs, feat, bg colour, ray_hit, the three z_unfilled) of a case, seeded."""
    seed = CR.case_seed(SR, C)
    b = CR.make_bufs(P_R, SR, seed=seed)
    feat = CR.make_feat(b, C, seed=seed)
    g = torch.Generator().manual_seed(4000 + seed)
    bgc = torch.rand(C, generator=g) if bg else None
    hit, zs = perspective_case(b, seed)
    return b, feat, bgc, hit, zs
