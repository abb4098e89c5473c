"""CPU checks of the DTU aggregator configuration (63-channel features, agg_intrp_order 1;
DESIGN.md section 31): the numpy restatement of tests/aggregate_dtu_ref.py against the reference's
own recorded outputs (tests/golden/aggregator_dtu.npz) and against oracle.aggregate, the emulated
kernel bugs against the tight bar, NeuralPoints.assemble_embedding, and the host layer's shapes
and refusals.  No GPU."""
import os

import numpy as np
import pytest
import torch

import aggregate_dtu_ref as DR
import aggregate_ref as AR
from formula import formula_params
from oracle import oracle as O

from pointnerf_amd import _lib as L
from pointnerf_amd.aggregator import PointAggregator, check_supported
from pointnerf_amd.neural_points import NeuralPoints
from pointnerf_amd.options import dtu_opt, dtu_script_opt, lego_opt


@pytest.fixture(scope="module")
def dtu(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "aggregator_dtu.npz"), allow_pickle=False))


def _restated(g, pre, E, order, dtype=np.float32):
    return DR.aggregate(DR.params_for(E, float(g["salt"])), g[pre + "sampled_color"][0], None,
                        g[pre + "sampled_dir"][0], g[pre + "sampled_conf"][0], g[pre + "sampled_embedding"][0],
                        g[pre + "sampled_xyz_pers"][0], g[pre + "sampled_xyz"][0], g[pre + "sample_pnt_mask"][0],
                        g[pre + "sample_loc"][0], g[pre + "sample_loc_w"][0], g[pre + "sample_ray_dirs"][0],
                        order=order, dtype=dtype)


# ------------------------------------------------------------------ restatement vs the reference's outputs
@pytest.mark.parametrize("pre, E, order", [("a_", 63, 2), ("a_", 63, 1), ("b_", 32, 1)])
def test_restatement_matches_reference_fixture(dtu, pre, E, order):
    """The bars test_oracle_golden.py uses for aggregator.npz."""
    g = dtu
    assert g[pre + "sampled_embedding"].shape == (1, 6, 10, 8, E)
    f, rv, w, cc = _restated(g, pre, E, order)
    assert np.array_equal(rv, g[pre + "ray_valid"][0])
    np.testing.assert_allclose(f, g[f"{pre}features_o{order}"][0], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(w, g[pre + "weight"][0], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(cc, g[pre + "conf_coefficient"][0], atol=1e-7, rtol=0)
    m = g[pre + "sample_pnt_mask"][0]
    # the edge cases the fixture forces
    assert not rv[0].any() and np.all(f[0] == 0) and not rv[1, 3] and np.all(f[1, 3] == 0)
    assert np.all(m[2].sum(-1) <= 1) and rv[2].any()


def test_fixture_orders_differ_where_they_must(dtu):
    """Order 1 against order 2 on the same inputs: another alpha, colours through a sigmoid."""
    f1, f2, rv = dtu["a_features_o1"][0], dtu["a_features_o2"][0], dtu["a_ray_valid"][0]
    assert np.abs(f1[rv][:, 0] - f2[rv][:, 0]).max() > 1e-3
    assert f1[rv][:, 1:].min() > -0.0011 and f1[rv][:, 1:].max() < 1.0011
    sig = 1.0 / (1.0 + np.exp(-f2[rv][:, 1:].astype(np.float64)))     # raw2out_color of order 2's colours
    np.testing.assert_allclose(f1[rv][:, 1:], sig * 1.002 - 0.001, atol=1e-6, rtol=0)
    assert np.abs(f1[rv][:, 1:] - f2[rv][:, 1:]).min() > 0.1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_equals_oracle_at_32_order_2(golden_dir, dtype):
    """Bit for bit, on the aggregator.npz inputs, in the same dtype."""
    g = np.load(os.path.join(golden_dir, "aggregator.npz"), allow_pickle=False)
    args = (formula_params(), g["sampled_color"][0], None, g["sampled_dir"][0], g["sampled_conf"][0],
            g["sampled_embedding"][0], g["sampled_xyz_pers"][0], g["sampled_xyz"][0], g["sample_pnt_mask"][0],
            g["sample_loc"][0], g["sample_loc_w"][0], g["sample_ray_dirs"][0])
    old = O.F32
    O.F32 = dtype
    try:
        want = O.aggregate(*args)
    finally:
        O.F32 = old
    got = DR.aggregate(*args, order=2, dtype=dtype)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------ the emulated bugs against the tight bar
def _over_tight(base, E, order, mut):
    """Worst err / tight bar of the (mutated) fp32 emulation against float64 over the feature blocks."""
    c = DR.case(base, E, order)
    ref, e, sc = DR.ref64_and_noise(base, E, order)
    res = AR.compare(c, ref, *DR.emulate(c, mut))
    assert not res["canary"], res["canary"]
    return max((res["err"][k] / AR.tight_bar(e[k], sc[k]), k) for k in ("alpha", "colour"))


CAUGHT_BY = {"pe_stride32": ("n257", 63, 2), "split_224": ("n65", 63, 2), "drop_ch62": ("geom", 63, 2),
             "alpha_per_pair": ("n33", 63, 1), "no_raw2out_color": ("conf_out", 63, 1)}


@pytest.mark.parametrize("base, E, order", [("n257", 63, 2), ("n33", 63, 1), ("geom", 64, 1), ("used", 33, 2)])
def test_correct_emulation_is_inside_the_tight_bar(base, E, order):
    ratio, blk = _over_tight(base, E, order, None)
    assert ratio <= 1.0 / DR.C_TIGHT + 1e-12, (ratio, blk)   # the fp32 restatement IS e_o32


@pytest.mark.parametrize("mut", DR.MUTATIONS)
def test_mutation_misses_the_tight_bar_by_ten_times(mut):
    assert set(CAUGHT_BY) == set(DR.MUTATIONS)
    base, E, order = CAUGHT_BY[mut]
    ratio, blk = _over_tight(base, E, order, mut)
    print(f"{mut} on {base}/E{E}o{order}: err / tight bar = {ratio:.3g} ({blk})")
    assert ratio >= 10.0, (mut, ratio, blk)


def test_cases_cover_what_they_claim():
    assert {DR.case(b, 63, 2).N for b in DR.BASES} >= {1, 31, 32, 33, 63, 64, 65, 257}
    for base, E, order in DR.CASES:
        c = DR.case(base, E, order)
        assert c.emb.shape == (c.N, E) and c.rows <= 200 and c.K == 8
    assert sorted(E for _, E in DR.WIDTHS if E != 63) == [33, 33, 64, 64]
    g = DR.case("geom", 63, 1)
    assert np.array_equal(g.xyz[g.pidx[0, 0]], g.sample_w[0])          # a point exactly at its sample
    u = DR.case("used", 63, 2)
    assert u.n_used_dev is not None and u.n_used_dev < u.used.shape[0]  # device count below capacity
    cf = DR.case("conf_out", 63, 2).conf
    assert (cf < 1e-4).any() and (cf > 1).any()


# ------------------------------------------------------------------ assemble_embedding
def _parts(n=5, F=56):
    g = torch.Generator().manual_seed(3)
    return (torch.rand((n, F), generator=g), torch.rand((n, 3), generator=g) + 10, torch.rand((n, 3), generator=g) + 20,
            torch.rand((n, 1), generator=g) * 0.5 + 30)


def test_assemble_embedding_scripts_order():
    feat, color, dirs, conf = _parts()
    emb, c, d, cf = NeuralPoints.assemble_embedding(dtu_script_opt(), feat, color, dirs, conf)
    assert emb.shape == (1, 5, 63)
    assert torch.equal(emb[0, :, :3], color) and torch.equal(emb[0, :, 3:6], dirs)
    assert torch.all(emb[0, :, 6] == 1.0)               # default_conf 1 replaces the conf
    assert torch.equal(emb[0, :, 7:], feat)
    assert torch.equal(c, color) and torch.equal(d, dirs) and torch.all(cf == 1.0) and cf.shape == (5, 1)


def test_assemble_embedding_modes_and_truncation():
    feat, color, dirs, conf = _parts(F=70)
    o = dtu_script_opt(point_conf_mode="1", point_features_dim=62, default_conf=-1.0)   # 56 + 3 + 3
    emb, c, d, cf = NeuralPoints.assemble_embedding(o, feat[:, :56], color, dirs, conf)
    assert emb.shape == (1, 5, 62) and torch.equal(emb[0, :, 6:], feat[:, :56]) and torch.equal(cf, conf)
    o = dtu_script_opt(point_conf_mode="0", default_conf=-1.0)
    emb, c, d, cf = NeuralPoints.assemble_embedding(o, feat[:, :56], color, dirs, conf)
    assert cf is None and torch.equal(emb[0, :, 6], conf[:, 0])
    # feat wider than point_features_dim is cut first (neural_points.py:481-482)
    o = lego_opt()
    emb, c, d, cf = NeuralPoints.assemble_embedding(o, feat, color, dirs, conf)
    assert emb.shape == (1, 5, 32) and torch.equal(emb[0], feat[:, :32]) and torch.equal(c, color)


def test_assemble_embedding_refusals():
    feat, color, dirs, conf = _parts()
    with pytest.raises(L.PnrError, match="point_features_dim"):
        NeuralPoints.assemble_embedding(dtu_script_opt(point_features_dim=64), feat, color, dirs, conf)
    with pytest.raises(L.PnrError, match="point_color_mode"):
        NeuralPoints.assemble_embedding(dtu_script_opt(point_color_mode="0", point_features_dim=63), feat, color,
                                        dirs, conf)
    with pytest.raises(L.PnrError, match="point_dir_mode"):
        NeuralPoints.assemble_embedding(dtu_script_opt(point_dir_mode="0"), feat, color, dirs, conf)


# ------------------------------------------------------------------ the host layer
def test_dtu_script_opt():
    o = dtu_script_opt()
    assert (o.point_features_dim, o.agg_intrp_order, o.default_conf, o.wcoord_query) == (63, 1, 1, 0)
    assert o.point_conf_mode == o.point_dir_mode == o.point_color_mode == "01"
    assert dtu_script_opt(agg_intrp_order=2).agg_intrp_order == 2
    assert (dtu_opt().point_features_dim, dtu_opt().agg_intrp_order) == (32, 2)   # unchanged


def test_point_aggregator_dtu_shapes_and_state_dict(dtu):
    agg = PointAggregator(dtu_script_opt())
    assert tuple(agg.block1[0].weight.shape) == (256, 501)
    params = DR.params_for(63, float(dtu["salt"]))
    assert params["block1.0.weight"].shape == (256, 501)
    missing, unexpected = agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    assert not missing and not unexpected
    assert (agg.E, agg.order, agg.split) == (63, 1, 441)
    specs = {n: (tuple(W.shape), b is not None) for n, W, b in agg._fp32_specs()}
    assert specs["w1af"] == ((256, 441), True) and specs["w1bf"] == ((256, 60), False)
    lego = PointAggregator(lego_opt())
    assert tuple(lego.block1[0].weight.shape) == (256, 284) and (lego.E, lego.order, lego.split) == (32, 2, 224)


def test_check_supported_dtu():
    check_supported(dtu_script_opt())
    check_supported(dtu_script_opt(agg_intrp_order=2))
    check_supported(lego_opt(point_features_dim=1))
    check_supported(lego_opt(point_features_dim=64))
    for bad, flag in ((dict(agg_intrp_order=0), "agg_intrp_order"), (dict(agg_distance_kernel="quadric"),
                      "agg_distance_kernel"), (dict(point_features_dim=65), "point_features_dim"),
                      (dict(point_features_dim=0), "point_features_dim"),
                      (dict(agg_intrp_order=1, shading_color_channel_num=3), "agg_intrp_order")):
        with pytest.raises(L.PnrError, match=flag):
            check_supported(dtu_script_opt(**bad))


def test_neural_points_width_and_bf16_refusals():
    """Both raised by the constructor before it builds its querier (which needs a GPU)."""
    o = dtu_script_opt()
    with pytest.raises(L.PnrError, match="point_features_dim is 63"):
        NeuralPoints(o, "cpu", torch.rand((7, 3)), torch.rand((1, 7, 32)))
    with pytest.raises(L.PnrError, match="bf16"):
        NeuralPoints(o, "cpu", emb_dtype=torch.bfloat16)


def test_training_and_bf16_packs_refused_before_any_launch():
    agg = PointAggregator(dtu_script_opt())
    for call in (lambda: agg.packed_train(h2=True), agg.packed_bf16, agg.packed_h2_train):
        with pytest.raises(L.PnrError, match="point_features_dim"):
            call()
    agg2 = PointAggregator(dtu_script_opt(point_features_dim=32))
    with pytest.raises(L.PnrError, match="agg_intrp_order"):
        agg2.packed_bf16()


def test_checkpoint_width_mismatch_names_both(tmp_path):
    from pointnerf_amd.checkpoint import load_ray_marching
    sd = {"neural_points.xyz": torch.rand((4, 3)), "neural_points.points_embeding": torch.rand((1, 4, 63))}
    p = str(tmp_path / "w.pth")
    torch.save(sd, p)
    with pytest.raises(L.PnrError, match=r"63 wide.*point_features_dim is 32"):
        load_ray_marching(p, dtu_opt(), "cpu")
    sd["aggregator.block1.0.weight"] = torch.zeros((256, 284))
    torch.save(sd, p)
    with pytest.raises(L.PnrError, match=r"284 inputs.*501"):
        load_ray_marching(p, dtu_script_opt(), "cpu")


def test_abi_structs_end_with_the_new_fields():
    assert L.ABI_VERSION >= 31 and L.lib().pnr_abi_version() == L.ABI_VERSION
    assert L.Points._fields_[-1][0] == "emb_dim" and L.Mlp._fields_[-1][0] == "intrp_order"
    assert L.Points().emb_dim == 0 and L.Mlp().intrp_order == 0      # the defaults: 32 wide, order 2
    p = L.Points(1, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None, None)
    assert p.emb_dim == 0                                             # a positionally built struct keeps working


def test_c_entry_points_refuse_wide_tables_where_they_must():
    lib, by = L.lib(), L.ctypes.byref
    FAKE = 0x1000
    pts = L.Points(8, FAKE, FAKE, FAKE)
    pts.emb_dim = 63
    s = L.Samples(None, None, 8, FAKE, FAKE, FAKE, FAKE, None, 1, 8)
    m16 = L.MlpBf16()
    rc = lib.pnr_aggregate_fwd_bf16(by(pts), by(s), by(m16), FAKE, None, None, FAKE, 1 << 20, None)
    assert rc == L.PNR_EINVAL and b"emb_dim" in lib.pnr_last_error()
    mlp = L.Mlp()
    for name, ctype in L.Mlp._fields_:
        if ctype is L.c_void_p:
            setattr(mlp, name, FAKE)
    mlp.intrp_order = 1
    pts.emb_dim = 0
    sv = L.AggSaved()
    rc = lib.pnr_aggregate_fwd_train(by(pts), by(s), by(mlp), by(sv), FAKE, None, None, FAKE, 1 << 30, None)
    assert rc == L.PNR_EINVAL and b"intrp_order" in lib.pnr_last_error()
    mlp.intrp_order = 3
    rc = lib.pnr_aggregate_fwd(by(pts), by(s), by(mlp), FAKE, None, None, FAKE, 1 << 30, None)
    assert rc == L.PNR_EINVAL and b"intrp_order 3" in lib.pnr_last_error()
    mlp.intrp_order = 1
    pts.emb_dim = 65
    rc = lib.pnr_aggregate_fwd(by(pts), by(s), by(mlp), FAKE, None, None, FAKE, 1 << 30, None)
    assert rc == L.PNR_EINVAL and b"emb_dim 65" in lib.pnr_last_error()
