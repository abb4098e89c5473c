"""CPU checks of tests/aggregate_ref.py: every case carries the edge it is named
for (counted from its arrays), the restated gather is pinned bitwise to
``oracle.gather`` + ``oracle.aggregate`` on a real query, the noise of fp32
arithmetic (``e_o32``) stays at or below a quarter of the project bar on every
case tests/test_gpu_aggregate_edges.py runs, and a numpy emulation of each
plausible kernel bug fails a named case by more than ten times the tight bar.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import aggregate_ref as AR
from formula import formula_params
from oracle import oracle as O
from scenes import oracle_points, scene


def _cdiv(a, b):
    return -(-a // b)


def _filled(c):
    return c.pidx >= 0


def _dist(c):
    """|xyz[pidx] - sample| of the filled slots."""
    m = _filled(c)
    d = np.linalg.norm(c.xyz[np.maximum(c.pidx, 0)].astype(np.float64) - c.sample_w[:, None, :], axis=-1)
    return d[m]


# ------------------------------------------------------------------ invariants
@pytest.mark.parametrize("name", AR.CASES)
def test_case_is_legal_and_seeded(name):
    """Every case is a legal pnr.h input (indices in range, lists inside their
    tables) and the same arrays on a second build."""
    c = AR.case(name)
    again = AR._BUILDERS[name]()
    for k, v in vars(c).items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, getattr(again, k)), k
    assert c.pidx.shape == (c.rows, c.K) and c.pidx.dtype == np.int32
    assert (c.pidx >= -1).all() and (c.pidx < c.N).all()
    assert c.xyz.shape == (c.N, 3) and c.emb.shape == (c.N, 32)
    n_eff = min(c.n_dev, c.n_max)
    if c.samp_list is not None:
        assert c.samp_list.shape[0] >= c.n_max and (c.samp_list >= 0).all() and (c.samp_list < c.rows).all()
        assert np.unique(c.samp_list).size == c.samp_list.size
    else:
        assert c.n_max <= c.rows
    rows = np.arange(c.rows)
    drow = (c.dir_map if c.dir_map is not None else rows) // c.dir_div
    assert drow.min() >= 0 and drow.max() < c.dirs.shape[0]
    if c.ray_cam is not None:
        assert c.ray_cam.shape[0] == c.dirs.shape[0] and c.ray_cam.max() < c.campos.shape[0]
    assert np.allclose(np.linalg.norm(c.dirs, axis=1), 1, atol=1e-6)
    if c.used is not None:
        n_used = c.used.shape[0] if c.n_used_dev is None else min(c.n_used_dev, c.used.shape[0])
        ref = np.unique(c.pidx[_filled(c)])
        assert np.array_equal(c.used[c.used_map[ref]], ref) and c.used_map[ref].max() < n_used
    assert n_eff >= 0


@pytest.mark.parametrize("name", [n for n in AR.CASES if n.split("_")[0] in ("count", "sched", "ndev", "list", "K")])
def test_default_population(name):
    """The stated defaults: neighbours 0.003 to 0.05 from the sample, about 55 % of
    the slots filled, slots filled in order, some samples without a neighbour."""
    c = AR.case(name)
    d = _dist(c)
    assert d.size and d.min() >= 0.003 - 1e-7 and d.max() <= 0.05 + 1e-7
    m = _filled(c)
    assert (m[:, 1:] <= m[:, :-1]).all(), "slots fill in order"
    if c.rows >= 63:
        assert 0.42 <= m.mean() <= 0.62
        assert (~m.any(1)).any(), "a sample without a neighbour"


@pytest.mark.parametrize("n", AR.COUNTS)
def test_count_cases(n):
    c = AR.case(f"count_{n}")
    assert c.n_max == c.n_dev == c.rows == n and c.samp_list is None and c.dir_map is None and c.dir_div == 1
    assert c.K == 8 and c.N == 257
    # on or next to a tile edge of 8 (k_pairs*), 16..128 (k_pairs_b) or 64 (k_color_h2, k_point_pre_h2)
    assert any(abs(n - t * q) <= 1 for t in (8, 16, 64, 128) for q in (0, 1, 2)) or n == 7


@pytest.mark.parametrize("n, tiles, regime", zip(AR.SCHEDULE, (256, 257, 527, 528, 532),
                                                 ("static", "one", "one", "xcd", "xcd")))
def test_schedule_regimes(n, tiles, regime):
    """aggregate_x3.hip: grid = min(tiles, 256); static up to the grid, one counter
    below 2 * grid + 16 tiles, eight per-XCD counters from there."""
    c = AR.case(f"sched_{n}")
    nt = _cdiv(c.n_max, AR.TILE_X3)
    grid = min(nt, 256)
    assert nt == tiles and c.N == 1024
    got = "static" if nt <= grid else ("xcd" if nt >= 2 * grid + 16 else "one")
    assert got == regime
    if n == 4249:
        assert nt % 8 != 0
    # every sample distinct: a swapped tile gives wrong rows, a skipped one leaves canaries
    assert np.unique(c.sample_w, axis=0).shape[0] == n
    r = AR.ref64_and_noise(f"sched_{n}")[0]
    wr = ~r["untouched"]
    assert np.unique(np.round(r["feat"][wr], 7), axis=0).shape[0] == wr.sum()
    assert wr.reshape(-1)[-(n % 8 or 8):].any(), "the last tile writes a row"


def test_device_counts():
    for nd in (0, 37, 100, 250):
        c = AR.case(f"ndev_{nd}")
        assert (c.n_max, c.n_dev) == (100, nd)
        r = AR.ref64_and_noise(c.name)[0]
        assert r["rows"].size == min(nd, 100) and r["untouched"][min(nd, 100):].all()
    c = AR.case("ndev_2050")
    assert (c.n_max, c.n_dev) == (4300, 2050) and _cdiv(2050, 8) == 257 and _cdiv(4300, 8) >= 528


def test_list_cases():
    c = AR.case("list_perm")
    sl = c.samp_list
    assert sl.size == 77 and (np.diff(sl) < 0).any() and (np.diff(np.sort(sl)) > 1).any()
    c = AR.case("list_dirmap")
    assert c.dir_map is not None and c.dir_div == AR.SR == 24
    assert ((c.dir_map // 24) != (np.arange(c.rows) // 24)).mean() > 0.9   # ignoring the map picks another row
    assert ((c.dir_map[c.samp_list] // 24) != c.samp_list % c.dirs.shape[0]).mean() > 0.9
    for div in (1, 5):
        c = AR.case(f"list_null_div{div}")
        assert c.samp_list is None and c.dir_map is None and c.dir_div == div and c.dirs.shape[0] == _cdiv(43, div)


def test_K_cases():
    for k in AR.K_CASES:
        c = AR.case(f"K_{k}")
        assert c.K == k and c.n_max == 41 and _filled(c).any()


@pytest.mark.parametrize("name", ["slots", "slots_xavier", "rw2c_point"])
def test_slot_patterns(name):
    c = AR.case(name)
    m, p, K, N = _filled(c), c.pidx, c.K, c.N
    assert c.n_max == 64 and K == 8
    tiles = m.reshape(8, 8, K)
    only = lambda k: m[:, k] & (m.sum(1) == 1)   # noqa: E731
    assert only(0).reshape(8, 8)[0].all() and only(K - 1).reshape(8, 8)[1].all()
    assert (tiles[2] == (np.arange(K) % 2 == 1)).all()                       # alternating
    assert (tiles[3][[0, 1, 5, 6, 7]] == (np.arange(K) < K // 2)).all()      # first half
    assert tiles[4].all() and np.all([np.unique(r).size == K for r in p[32:40]])   # all eight, distinct
    assert not tiles[3][2:5].any() and tiles[3][[1, 5]].any()                # all empty in mid-tile
    assert not tiles[6].any()                                                # a wholly empty tile
    assert np.all([m[r].all() and np.unique(p[r]).size == 1 for r in c.edges["onepoint"]])   # duplicates
    # point 0 a real neighbour beside empty slots (the clamped row of those slots)
    r0 = [r for r in range(64) if (p[r] == 0).any()]
    assert r0 == sorted(c.edges["point0"]) and all((p[r] == -1).any() and p[r, 0] == -1 for r in r0)
    assert sorted(r for r in range(64) if (p[r] == N - 1).any()) == sorted(c.edges["pointlast"])
    # holes before a filled slot; buckets by "last filled slot + 1" differ from buckets by count
    hole = (~m[:, :-1] & (np.cumsum(m[:, ::-1], 1)[:, ::-1][:, 1:] > 0)).any(1)
    assert hole.sum() >= 20
    cnt = m.sum(1)
    kt_cnt = np.where(cnt <= 1, 1, np.where(cnt <= 2, 2, np.where(cnt <= 4, 4, 8)))
    assert (AR.bucket_kt(m)[m.any(1)] > kt_cnt[m.any(1)]).sum() >= 16
    assert set(AR.bucket_kt(m)[m.any(1)]) == {1, 4, 8} or set(AR.bucket_kt(m)[m.any(1)]) == {1, 2, 4, 8}
    if name == "rw2c_point":   # samples whose slot 0 is empty while later slots are filled
        assert c.rw2c is not None and (~m[:, 0] & m.any(1)).sum() >= 16
        assert not np.allclose(c.rw2c[0], np.eye(3), atol=0.1)


@pytest.mark.parametrize("name", ["geom", "geom_xavier"])
def test_geometry(name):
    c = AR.case(name)
    e, p = c.edges, c.pidx
    co = [k for k in range(c.K) if p[e["coincident"], k] >= 0 and
          np.array_equal(c.xyz[p[e["coincident"], k]], c.sample_w[e["coincident"]])]
    assert len(co) == 1 and (p[e["coincident"]] >= 0).sum() >= 4
    r = e["all_coincident"]
    assert (p[r] >= 0).all() and np.unique(p[r]).size == c.K
    assert all(np.array_equal(c.xyz[q], c.sample_w[r]) for q in p[r])
    for key, want in (("far03", 0.3), ("far2", 2.0)):
        r = e[key]
        d = np.linalg.norm(c.xyz[p[r][p[r] >= 0]].astype(np.float64) - c.sample_w[r], axis=1)
        assert np.isclose(d.max(), want, rtol=1e-3) and (d < 0.06).sum() == d.size - 1
    # the coincident pair takes the 1 / max(|d|, 1e-6) clamp: weight ~ 1 next to ~1e-4
    w = AR.ref64_and_noise(name)[0]["weight"]
    assert w[e["coincident"]].max() > 0.999 and np.allclose(w[e["all_coincident"]], 0.125)


def test_tables():
    c = AR.case("conf_range")
    used = c.conf[c.pidx[_filled(c)]]
    assert (used < 1e-4).sum() > 10 and (used > 1).sum() > 10 and ((used >= 1e-4) & (used <= 1)).sum() > 10
    assert AR.case("conf_null").conf is None and AR.case("color_null").color is None
    assert AR.case("dir_null").dir is None and AR.case("dir_null").color is not None
    a, b = AR.case("pers_given"), AR.case("pers_null")
    assert a.pers is not None and b.pers is None and np.array_equal(a.xyz, b.xyz) and np.array_equal(a.pidx, b.pidx)
    assert np.array_equal(a.pers, O.w2pers(a.xyz, a.campos[0], a.camrot[0]))
    c = AR.case("two_cams")
    rows = np.arange(c.rows)
    cam = c.ray_cam[rows // c.dir_div]
    assert c.campos.shape == (2, 3) and min((cam == 0).sum(), (cam == 1).sum()) >= 10
    assert not np.allclose(c.camrot[0], c.camrot[1], atol=0.1)
    for ci in (0, 1):   # sample_p belongs to the sample's own camera
        assert np.array_equal(c.sample_p[cam == ci], O.w2pers(c.sample_w[cam == ci], c.campos[ci], c.camrot[ci]))
    c = AR.case("rw2c_uniform")
    assert c.Rw2c is not None and c.rw2c is None and not np.allclose(c.Rw2c, np.eye(3), atol=0.1)
    assert np.allclose(c.Rw2c @ c.Rw2c.T, np.eye(3), atol=1e-6)
    c = AR.case("act_relu")
    assert (c.neg_slope, c.act_super) == (0.0, 0) and AR.ref64_and_noise("act_relu")[2]["alpha"] > 0.01
    c = AR.case("act_lego")
    assert (c.neg_slope, c.act_super) == (0.01, 1)


def test_used_subsets():
    c = AR.case("used_subset")
    ref = np.unique(c.pidx[_filled(c)])
    assert np.array_equal(c.used, ref) and ref.size < c.N // 2 and c.n_used_dev is None
    assert (c.used_map >= 0).sum() == ref.size
    # the clamped row of the empty slots is itself unreferenced: used_map[0] = -1
    assert c.used_map[0] == -1 and (~_filled(c)).any()
    assert (c.used_map[ref] != ref).mean() > 0.9      # ignoring the map picks another P1 row
    c = AR.case("used_dev")
    assert c.n_used_dev == np.unique(c.pidx[_filled(c)]).size < c.used.shape[0]


@pytest.mark.parametrize("n", AR.N_TAILS)
def test_point_table_tails(n):
    c = AR.case(f"ntail_{n}")
    assert c.N == n and np.array_equal(np.unique(c.pidx[_filled(c)]), np.arange(n))   # every point referenced
    if n == 1:
        assert (~_filled(c)).any() and _filled(c).any(1).all()


# ------------------------------------------------- pinned to the oracle's gather
def test_restated_gather_equals_oracle_gather_bitwise():
    """On a scene() query, in fp32: reference() == oracle.gather + oracle.aggregate."""
    sc = scene(20000, H=24, W=24, default_conf=None)
    params = formula_params(salt=0.3)
    q = O.query_points(sc["opt"], sc["xyz"], sc["campos"], sc["camrot"], sc["raydir"], near=2.0, far=6.0)
    g = O.gather(oracle_points(sc), q["sample_pidx"], sc["campos"], sc["camrot"])
    want, rv, w, cc = O.aggregate(params, g["sampled_color"], None, g["sampled_dir"], g["sampled_conf"],
                                  g["sampled_embedding"], g["sampled_xyz_pers"], g["sampled_xyz"],
                                  g["sample_pnt_mask"], q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"])
    R, SR, K = q["sample_pidx"].shape
    assert rv.sum() > 300
    c = SimpleNamespace(
        name="scene", N=sc["xyz"].shape[0], K=K, rows=R * SR, xyz=sc["xyz"], emb=sc["emb"], color=sc["color"],
        dir=sc["dir"], conf=sc["conf"].reshape(-1), pers=None, rw2c=None, Rw2c=None, campos=sc["campos"][None],
        camrot=sc["camrot"][None], ray_cam=None, pidx=q["sample_pidx"].reshape(R * SR, K), pair_mask=None,
        sample_w=q["sample_loc_w"].reshape(-1, 3), sample_p=q["sample_loc"].reshape(-1, 3),
        dirs=np.ascontiguousarray(sc["raydir"][q["ray_mask"] > 0]), dir_map=None, dir_div=SR, samp_list=None,
        n_max=R * SR, n_dev=R * SR, used=None, used_map=None, n_used_dev=None, neg_slope=0.01, act_super=1,
        weights=("formula", 0.3), edges={})
    got = AR.reference(c, np.float32)
    assert got["feat"].dtype == np.float32
    assert np.array_equal(got["feat"].reshape(R, SR, 129), want)
    assert np.array_equal(~got["untouched"], rv.reshape(-1))
    assert np.array_equal(got["weight"].reshape(R, SR, K), w) and np.array_equal(got["conf"].reshape(R, SR, K), cc)
    # the pair-table layout (pnr_aggregate_fwd_masked) restates the same numbers
    m = AR.reference(AR.to_masked(AR.case("slots")), np.float32)
    p = AR.reference(SimpleNamespace(**dict(vars(AR.case("slots")),
                                            pers=O.w2pers(AR.case("slots").xyz, AR.case("slots").campos[0],
                                                          AR.case("slots").camrot[0]))), np.float32)
    for k in ("feat", "untouched", "weight", "conf"):
        assert np.array_equal(m[k], p[k]), k


# ------------------------------------------------------------ noise of fp32
@pytest.mark.parametrize("name, masked", [(n, False) for n in AR.CASES] + [(n, True) for n in AR.MASKED])
def test_fp32_noise_is_a_quarter_of_the_bar_or_less(name, masked):
    """e_o32 = |reference(float32) - reference(float64)| per block against the project
    bar 1e-4 + 1e-4 |ref|: correct fp32 arithmetic meets the bar four times over on
    every case, so the tight bar of the GPU test (8 e_o32) sits well inside it."""
    _, e, sc, nr = AR.ref64_and_noise(name, masked)
    print(f"{name}: " + "  ".join(f"{k} e_o32 {e[k]:.2e} ({nr[k]:.4f} of the bar)" for k in AR.BLOCKS))
    for k in AR.BLOCKS:
        assert nr[k] <= 0.25, (name, k, e[k], nr[k])
        assert AR.tight_bar(e[k], sc[k]) <= 0.25 * (AR.ATOL + AR.RTOL * sc[k]) or sc[k] == 0.0, (name, k)


# ------------------------------------------------------------- sensitivity
def _worst_over_tight(name, mut):
    """An emulated kernel (bug ``mut``, fp32) against the float64 reference: the worst
    err / tight bar over the blocks (inf on a canary violation)."""
    c = AR.case(name)
    ref, e, sc, _ = AR.ref64_and_noise(name)
    res = AR.compare(c, ref, *AR.emulate(c, mut))
    if res["canary"]:
        return float("inf"), res["canary"][0]
    worst = max(((res["err"][k] / AR.tight_bar(e[k], sc[k]) if sc[k] > 0 else 0.0), k) for k in res["err"])
    return worst


def _numeric_over_tight(name, mut):
    """The same emulation judged by numbers alone: the worst err / tight bar over the
    rows that the emulated kernel and the reference both write (canaries set aside)."""
    c = AR.case(name)
    ref, e, sc, _ = AR.ref64_and_noise(name)
    of, ow, _oc = AR.emulate(c, mut)
    both = ~ref["untouched"] & (of[:c.n_max, 0] != AR.CANARY_FEAT)
    d = np.abs(of[:c.n_max][both].astype(np.float64) - ref["feat"][both])
    wrote = ow[ref["rows"], 0] != AR.CANARY_W
    dw = np.abs(ow[ref["rows"]][wrote].astype(np.float64) - ref["weight"][wrote])
    errs = dict(alpha=d[:, 0].max() if d.size else 0.0, colour=d[:, 1:].max() if d.size else 0.0,
                weight=dw.max() if dw.size else 0.0)
    return max(((errs[k] / AR.tight_bar(e[k], sc[k]) if sc[k] > 0 else 0.0), k) for k in errs)


@pytest.mark.parametrize("name", AR.SMALL)
def test_correct_emulation_passes(name):
    """The unmutated fp32 emulation meets the tight bar and the canaries on every case
    (its error is e_o32 itself)."""
    ratio, where = _worst_over_tight(name, None)
    assert ratio <= 1.0 / AR.C_TIGHT + 1e-12, (name, ratio, where)


# mutation -> the cases that must catch it
CAUGHT_BY = {
    "drop_kt": ("slots", "slots_xavier"),
    "skip_last_tile": ("count_9", "count_65"),
    "shift_tile": ("count_17",),
    "ignore_mask": ("slots", "ntail_1"),
    "conf_unclamped": ("conf_range",),
    "unnormalised": ("count_9",),
    "uniform_rw2c": ("rw2c_point", "rw2c_point_xavier"),
    "view_own_matrix": ("rw2c_point",),
    "dirs_no_map": ("list_dirmap", "list_null_div5"),
    "cam0": ("two_cams",),
    "ignore_n_dev": ("ndev_37", "ndev_0"),
    "ignore_used_map": ("used_subset", "used_dev"),
}


# caught by a canary first, and by the tight bar itself as well: a dropped slot (the
# alternating and point-0 rows still have a neighbour left) and the clamped row 0
# blended into samples that keep their own neighbours.  skip_last_tile and ignore_n_dev
# change which rows are written and nothing else, so only the canaries can see them.
NUMERIC_TOO = {("drop_kt", "slots"), ("drop_kt", "slots_xavier"), ("ignore_mask", "slots")}


def test_every_mutation_is_listed():
    assert set(CAUGHT_BY) == set(AR.MUTATIONS)


@pytest.mark.parametrize("mut", AR.MUTATIONS)
def test_mutation_fails_its_cases_by_ten_times_the_tight_bar(mut):
    for name in CAUGHT_BY[mut]:
        ratio, where = _worst_over_tight(name, mut)
        num, blk = _numeric_over_tight(name, mut)
        print(f"{mut} on {name}: err / tight bar = {ratio:.3g} ({where}); by numbers alone, on the rows both "
              f"write: {num:.3g} ({blk})")
        assert ratio >= 10.0, (mut, name, ratio, where)
        if (mut, name) in NUMERIC_TOO:
            assert num >= 10.0, (mut, name, num, blk)
