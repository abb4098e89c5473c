"""CPU checks of tests/nr_ref.py, the float64 reference of
tests/test_gpu_neural_render_edges.py: the masked restatement is the plain one bit
for bit, every case reaches the tile loop / plan / scale it is named for, the fp32
restatement under frozen masks stays inside the project bar on every case (so the
reference alone never uses the bar up), and a float32 emulation of each plausible
kernel bug misses the tight bar of a named case by more than ten times.
"""
import copy
import math

import pytest
import torch

import nr_ref as NR

NAMES = [c[0] for c in NR.CASES]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_render_ref_is_neural_render_torch_bitwise(dtype):
    for name in ("two_129", "stage_0up"):
        m, x, _ = NR.case_inputs(name)
        md = copy.deepcopy(m).to(dtype)
        with torch.no_grad():
            want = NR.neural_render_torch(md, x.to(dtype))
            got, zs = NR.render_ref(md, x.to(dtype))
            again, _ = NR.render_ref(md, x.to(dtype), [z > 0 for z in zs])
        assert got.dtype == dtype and torch.equal(got, want)
        # where(z > 0, z, 0.2 z) is leaky_relu itself
        assert torch.equal(again, want)
        assert zs[0].shape == (1, 64) + x.shape[1:3] and zs[1].shape == (1, 32) + x.shape[1:3]


def test_cases_are_seeded_and_distinct():
    a = NR.case_inputs("two_129")
    NR._INPUTS.pop("two_129")
    b = NR.case_inputs("two_129")
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for pa, pb in zip(a[0].parameters(), b[0].parameters()):
        assert torch.equal(pa, pb)
    assert not torch.equal(NR.case_inputs("x_zero")[0].conv_rgb[0].weight, a[0].conv_rgb[0].weight)
    assert len(set(NAMES)) == len(NAMES)


@pytest.mark.parametrize("name", [c[0] for c in NR.CASES if c[3] != NR.ONE])
def test_scaled_cases_pick_three_different_shifts(name):
    """Hole 1 stays exercised: the three forward stacks get pairwise different fp32h2
    shifts, and the three transposed backward stacks do too."""
    fwd, bwd = NR.shifts(name)
    print(name, "forward shifts", fwd, "transposed", bwd)
    assert len(set(fwd)) == 3 and len(set(bwd)) == 3
    want = {NR.UP1: [-9, -6, -10], NR.UP0: [-6, -9, -7]}[NR.CASE[name][3]]
    assert fwd == want and bwd == want


def test_default_init_hides_the_stage_scale():
    """Why the parametrised factors are needed: nn.Conv2d's default init gives stages 1
    and 2 the same shift."""
    fwd, bwd = NR.shifts("two_129")
    assert fwd[1] == fwd[2] and bwd[1] == bwd[2]


def test_cases_reach_what_they_are_named_for():
    hw = {c[0]: (c[1], c[2]) for c in NR.CASES}
    t = lambda n, ro: NR.tiles(*hw[n], ro)   # noqa: E731
    # tall_5: every fp32 workgroup takes 3 or 4 tiles, h2 workgroups a second one
    assert t("tall_5", 1) == 3000 and NR.cdiv(3000, NR.GRID_F32) == 4
    assert t("tall_5", NR.RO_H2) == 1500 > NR.GRID_H2 and t("tall_5", NR.RO_H2_DX) == 3000
    assert 3000 * 5 > NR.ABSMAX_GRID_PX
    assert hw["tall_5_top4"] == hw["tall_5"] and NR.CASE["tall_5_top4"][4][1] == 2 * (1500 - NR.GRID_H2) - 1
    # tall_130: a 2-pixel second segment, second tiles in every kernel, both 171-split plans
    for n in ("tall_130", "tall_130_1up"):
        H, W = hw[n]
        assert W - NR.SEG == 2 and t(n, NR.RO_H2) == 1100 > NR.GRID_H2 and t(n, 1) == 2200 > NR.GRID_F32
        assert NR.cdiv(H * W, 8 * 32) > 171 and NR.cdiv(H * W, 8 * 64) > 171       # the plan's split ceiling
        assert NR.wgrad_plan(H * W, 64)[1] > 8 * 64 and H * W > NR.RGB_GRAD_H2_GRID_PX
    # segs_3: the d x convolution's workgroups change segment on their second tile
    H, W = hw["segs_3"]
    assert NR.cdiv(W, NR.SEG) == 3 and t("segs_3", NR.RO_H2_DX) == 1035 > NR.GRID_H2 and NR.GRID_H2 % 3 == 1
    assert NR.cdiv(H * W, 8 * 64) > 171
    # the small shapes
    assert hw["px_1"] == (1, 1) and hw["row_128"] == (1, NR.SEG) and hw["two_129"] == (2, NR.SEG + 1)
    assert hw["row_257"][0] < NR.RO_H2 and hw["three_257"][0] % NR.RO_H2 == 1 and hw["five_127"][0] % NR.RO_H2 == 1
    assert [NR.wgrad_plan(n, 32) for n in (255, 256, 257)] == [(1, 256), (1, 256), (2, 160)]
    assert [NR.wgrad_plan(n, 64)[0] for n in (255, 256, 257)] == [1, 1, 1]
    assert NR.wgrad_plan(3 * 257, 32) == (4, 224) and 3 * 257 % 224
    for n in ("x_zero", "x_zero_b0"):
        assert not NR.case_inputs(n)[1].any()
    assert not NR.case_inputs("g_zero")[2].any()
    m = NR.case_inputs("x_zero_b0")[0]
    assert not m.conv_layers[0].bias.any() and not m.conv_layers[1].bias.any() and m.conv_rgb[0].bias.any()
    assert all(not z.any() for z in NR.forward64("x_zero_b0"))      # exact zeros: the z >= 0 / z > 0 edge
    assert NR.case_inputs("x_zero")[0].conv_layers[0].bias.any()


# ------------------------------------------------------------ noise of fp32
@pytest.mark.parametrize("name", NAMES)
def test_fp32_noise_under_frozen_masks_is_inside_the_bar(name):
    """e32 = max|fp32 restatement - fp64 restatement| with both under the fp64 forward's
    masks, per entry, against the project bar; and the share of pre-activations whose
    sign the unfrozen fp32 forward gets differently, against a tenth of the 1e-4 the GPU
    test allows a kernel."""
    masks = NR.masks64(name)
    ref, e32 = NR.ref64_and_noise(name, masks)
    for k in ("out",) + NR.GRADS:
        scale = ref[k].abs().max().item()
        bar = NR.project_bar(k, scale)
        print(f"{name} {k}: e32 {e32[k]:.3e}  max|ref| {scale:.3e}  e32 / bar {e32[k] / bar if bar else 0.0:.4f}")
        assert e32[k] <= bar, (name, k, e32[k], bar)
        assert math.isfinite(scale)
    m, x, _ = NR.case_inputs(name)
    with torch.no_grad():
        z32 = NR.render_ref(m, x)[1]
    for s in (0, 1):
        flips = ((z32[s] > 0) != masks[s])
        share = flips.double().mean().item()
        z64 = ref[f"z{s}"]
        print(f"{name} z{s}: e32 {e32[f'z{s}']:.3e}  max|z| {z64.abs().max().item():.3e}  fp32 sign flips {share:.2e}")
        assert share <= 1e-5, (name, s, share)
        # a flip of the unfrozen forward sits within the frozen forwards' noise of 0 (z1 also
        # carries the flips of z0, so only stage 0 is a clean statement)
        if s == 0:
            assert (z64[flips].abs() <= 8 * e32["z0"]).all()


# ------------------------------------------------------------- sensitivity
# mutation -> the case that must catch it
CAUGHT_BY = {
    "scale_fwd": "stage_1up",
    "scale_bwd": "stage_1up",
    "acc_not_cleared": "tall_5",
    "stale_x0": "segs_3",
    "halo_col128": "two_129",
    "drop_odd_row": "three_257",
    "drop_last_split": "row_257",
    "bias_octet": "row_128",
    "mask_ge": "x_zero_b0",
    "amax_last_tile": "tall_5_top4",
}


def test_every_mutation_is_listed():
    assert set(CAUGHT_BY) == set(NR.MUTATIONS)


@pytest.mark.parametrize("mut", NR.MUTATIONS)
def test_mutation_misses_the_tight_bar_by_ten_times(mut):
    """The unmutated float32 emulation meets the tight bar of the mutation's case, the
    mutated one misses it by more than 10x on at least one entry."""
    name = CAUGHT_BY[mut]
    masks = NR.masks64(name)
    ref, e32 = NR.ref64_and_noise(name, masks)
    ok, where_ok = NR.worst_over_tight(NR.emulate(name, masks), ref, e32)
    bad, where = NR.worst_over_tight(NR.emulate(name, masks, mut), ref, e32)
    print(f"{mut} on {name}: err / tight bar = {bad:.3g} ({where}); unmutated {ok:.3g} ({where_ok})")
    assert ok <= 1.0, (name, ok, where_ok)
    assert bad > 10.0, (mut, name, bad, where)
