"""CPU side of tests/test_gpu_objective.py: on every case of tests/objective_ref.py,
correct fp32 arithmetic -- the restatement, or an emulation of the kernel's own order
of operations -- is inside the bar the GPU test asks of the kernel, the cases reach
the edges they are meant to reach, and a wrong edge leaves the bar.

Worst ratios of the emulations with their cases (1.0 = the bar):
  sparse loss   value 0.166 (sr65_k8_n200_oob)  d_conf 0.115 (sr128_k16_n5000): fp32 weights,
                2^38 fixed point, fp64 sums; w_fix / 2^38 against float64 at 9.7e-4 of its
                allowance (sr65_k8_n5000_null)
  zero-one      value 0.205 (n5000_own_e7)  d_conf 0.462 whole and without point 0 (n8_big):
                k_zero_one_part / _final's summation order in fp32
  rgb head      1 / C_TIGHT by construction: the fp32 restatement is e_o32
"""
import numpy as np
import pytest
import torch

import loss_ref as LR
import objective_ref as OR

F32 = np.float32


# ------------------------------------------------------------------ A. sparse loss
def test_sparse_cases_cover_the_issue():
    cs = list(OR.SPARSE_CASES.values())
    assert {(c[0], c[1]) for c in cs} == {(1, 1), (63, 3), (64, 8), (65, 8), (80, 8), (128, 16)}
    assert {c[2] for c in cs} >= {1, 37, 255, 256, 257, 513, 5000}
    assert (128, 16, 1) in {c[:3] for c in cs}
    assert {c[3] for c in cs} == {"uniform", "low", "high", "null"}
    assert {c[4] for c in cs} == {None, "R0", "novalid", "oob"}
    # SR > 64 with rays filled past slot 64: the second pass of the slot loop
    b = OR.sparse_case("sr128_k16_n5000")["bufs"]
    assert int((b["n_filled"][b["ray_vcnt"] > 0] > 64).sum()) > 3
    # the refusal's R: one pair over the range, far more rays than the buffers hold
    assert (OR.SPARSE_MAX_PAIRS // (128 * 16) + 1) * 128 * 16 > OR.SPARSE_MAX_PAIRS


@pytest.mark.parametrize("name", sorted(OR.SPARSE_CASES))
def test_sparse_fp32_emulation_is_inside_the_bars(name):
    c = OR.sparse_case(name)
    r64, r32 = OR.sparse_reference(c, torch.float64), OR.sparse_reference(c, torch.float32)
    wfix = OR.wfix_from_weights(r32["w"].numpy(), c["ref_bufs"], c["N"])
    loss, d, _ = OR.sparse_from_wfix(wfix, c["conf"])
    LR.within(loss, r64["loss"], r32["loss"], f"RATIO sparse {name} loss")
    gathered = r64["pairs"].numpy() > 0
    if c["conf"] is None:                         # forward only: the backward refuses a NULL conf
        d = np.zeros(c["N"], F32)
    LR.within(d, r64["d_conf"], r32["d_conf"], f"RATIO sparse {name} d_conf")
    assert (d[~gathered] == 0).all() and (wfix[~gathered] == 0).all()
    if c["conf"] is not None and gathered.any():
        assert (d[gathered] != 0).all()          # straight-through: no clamp mask, at any conf
    err = np.abs(wfix / OR.W_SCALE - r64["W"].numpy())
    bar = OR.wfix_bar(r64)
    assert (err <= bar).all(), (name, float((err / np.maximum(bar, 1e-300)).max()))
    if gathered.any():
        print(f"RATIO sparse {name} w_fix err/bar {float((err[gathered] / bar[gathered]).max()):.3e}")
    if c["conf"] is None:                         # sum W f(1) / (sum W + 1e-6)
        W = r64["W"].double()
        assert float(r64["loss"]) == pytest.approx(float(W.sum() * abs(1 - np.exp(-2.0)) / (W.sum() + 1e-6)), rel=1e-12)
        assert not r64["d_conf"].any()
    if c["R"] == 0 or name.endswith("novalid"):
        assert float(r64["loss"]) == 0.0 and loss == 0 and not wfix.any() and not d.any()
    if c["N"] == 1 and c["R"]:
        assert int(r64["pairs"][0]) == int((OR.dense_pidx(c["ref_bufs"]) >= 0).sum()) > 1000


def test_sparse_out_of_range_entries_count_as_empty():
    c = OR.sparse_case("sr65_k8_n200_oob")
    assert int((c["bufs"]["pidx"] >= c["N"]).sum()) > 100 and int((c["ref_bufs"]["pidx"] >= c["N"]).sum()) == 0
    assert torch.equal(c["bufs"]["pidx"][c["bufs"]["pidx"] < c["N"]], c["ref_bufs"]["pidx"][c["bufs"]["pidx"] < c["N"]])


def test_sparse_slot_stride_mutation_leaves_the_bar():
    """A slot loop striding 65 instead of 64 drops slot 64 .. and shifts the rest: W
    changes by far more than check 2 allows wherever a ray is filled past slot 64."""
    c = OR.sparse_case("sr128_k16_n5000")
    r64 = OR.sparse_reference(c, torch.float64)
    b = c["ref_bufs"]
    w = r64["w"].clone()
    keep = torch.zeros(b["SR"], dtype=torch.bool)
    keep[torch.cat([torch.arange(l, b["SR"], 65) for l in range(64)])] = True
    w[:, ~keep] = 0
    wfix = OR.wfix_from_weights(w.float().numpy(), b, c["N"])
    assert (np.abs(wfix / OR.W_SCALE - r64["W"].numpy()) > OR.wfix_bar(r64)).any()


# -------------------------------------------- B. point counts and zero-one loss
@pytest.mark.parametrize("K", sorted(OR.COUNT_CASES))
def test_point_counts_reference_is_the_brute_force_count(K):
    c = OR.count_case(K)
    assert set(c["n_dev"]) == {0, 1, c["S"] // 2, c["S"], c["S"] + 5, -3}
    for n in c["n_dev"]:
        want = c["prefill"].copy()
        for i in range(min(max(n, 0), c["S"])):
            for p in c["pidx"][i]:
                if p >= 0:
                    want[p] += 1
        assert np.array_equal(OR.count_reference(c, n), want)
    assert not np.array_equal(OR.count_reference(c, c["S"]), OR.count_reference(c, c["S"] // 2))
    assert np.array_equal(OR.count_reference(c, -3), c["prefill"])


def test_zero_one_cases_cover_the_issue():
    cs = OR.ZO_CASES
    assert {v[0] for v in cs.values()} >= {1, 511, 512, 513, 5000}
    assert {v[1] for v in cs.values()} == {1e-3, 1e-2}
    assert {(v[2], v[3]) for v in cs.values()} >= {(True, 0), (False, 7), (True, 3000), (False, 4000), (False, 0)}
    for eps in (1e-3, 1e-2):
        lo, hi = OR.zo_bounds(eps)
        # torch.clamp rounds its Python bounds to fp32: the same numbers the kernel compares with
        assert lo == F32(eps) and hi == F32(1 - eps)
        pl = OR.zo_planted(eps)
        assert len(set(pl.tolist())) == pl.size == 15
        for b in (F32(1e-4), lo, hi, F32(1)):
            assert (pl == b).sum() == 1 and (pl < b).any() and (pl > b).any()
    big = OR.zo_case("n8_big")
    assert big["E"] == 24576 * 1024 > 2 ** 24 and big["empty"] > 10 ** 6
    assert OR.zo_case("n512_rvalid0")["E"] == 0


@pytest.mark.parametrize("name", sorted(OR.ZO_CASES))
def test_zero_one_kernel_order_emulation_is_inside_the_bars(name):
    c = OR.zo_case(name)
    loss64, d64 = OR.zo_truth(c)
    loss32, d32 = OR.zo_yardstick(c)
    out, d = OR.zo_emulate(c)
    LR.within(out[0], loss64, loss32, f"RATIO zero_one {name} loss")
    LR.within(d, d64, d32, f"RATIO zero_one {name} d_conf")
    LR.within(d[1:], d64[1:], d32[1:], f"RATIO zero_one {name} d_conf[1:]")
    zero = OR.zo_must_be_zero(c)
    assert (d[zero] == 0).all() and (d32[zero] == 0).all()
    lo, hi = OR.zo_bounds(c["eps"])
    if c["N"] >= 32 and c["E"] > 0:
        # the planted edges: on the bound the gradient passes, one fp32 step outside it does not
        conf, nz = c["conf"], ~zero
        for b, inside in ((lo, np.inf), (hi, -np.inf)):
            at = int(np.flatnonzero(conf[1:16] == b)[0]) + 1
            assert nz[at] and nz[int(np.flatnonzero(conf[1:16] == np.nextafter(b, F32(inside)))[0]) + 1]
            assert zero[int(np.flatnonzero(conf[1:16] == np.nextafter(b, F32(-inside)))[0]) + 1]
        assert zero[1:16][conf[1:16] >= 1].all() and zero[1:16][conf[1:16] <= F32(1e-4)].all()
    if c["E"] == 0:
        assert out[0] == 0 and out[2] == 0 and not d.any() and loss64 == 0
    elif name != "n8_big":
        assert out[1] == c["empty"] and out[2] == c["E"]
    else:
        # E and the counts' sum are fp32 in the kernel: above 2^24 the empty count is off by a few entries
        assert out[2] == c["E"] and 0 < abs(float(out[1]) - c["empty"]) <= 8
        print(f"RATIO zero_one n8_big empty: fp32 {float(out[1]):.0f} exact {c['empty']} "
              f"(relative {abs(float(out[1]) - c['empty']) / c['empty']:.2e})")
    if name == "n513_p0_nothing":
        assert d[0] == 0 and d64[0] == 0
    if c["empty"] >= 3000 and c["N"] > 8:    # point 0 carries the empty entries: why d_conf is judged without it as well
        assert c["counts"][0] + c["empty"] > 50 * c["counts"][1:].max()


def test_zero_one_mask_mutation_leaves_the_bar():
    """cc <= 1 - eps turned into cc < 1 - eps zeroes the entry planted on the bound."""
    c = OR.zo_case("n513_own_e3000")
    _, d64 = OR.zo_truth(c)
    at = int(np.flatnonzero(c["conf"] == OR.zo_bounds(c["eps"])[1])[0])
    assert d64[at] != 0 and not OR.zo_must_be_zero(c)[at]


# ------------------------------------------------------------------ C. rgb head
def test_head_cases_cover_the_issue():
    cs = OR.HEAD_CASES.values()
    assert {c[0] for c in cs} == {0, 1, 7, 8, 9, 4095, 4096, 4097, 16400}
    assert {c[1] for c in cs} == {"null", "eq", "m9", "p5", "zero"}
    assert {c[2] for c in cs} == {129, 136} and {c[3] for c in cs} == {0, 1} and {c[4] for c in cs} == {0.1, 1.0}
    assert {c[3] for c in cs if c[5]} == {0, 1}
    assert 4095 < OR.HEAD_BWD_BLOCKS * 8 < 4097 and 16400 > 2048 * 8    # blocks without a row; the forward's second pass


@pytest.mark.parametrize("name", sorted(OR.HEAD_CASES))
def test_head_fp32_restatement_is_inside_the_bar(name):
    c = OR.head_case(name)
    r64, e, sc = OR.head_noise(c)
    r32 = OR.head_reference(c, F32)
    assert r64["out"].shape == (c["n"], 4) and r64["d_feat"].shape == (c["n"], 129)
    for k in OR.HEAD_TENSORS:
        err, ratio = OR.head_ratio(r32[k], r64[k], e[k], sc[k])
        print(f"RATIO head host {name:18s} {k:7s} err {err:.3e}  e_o32 {e[k]:.3e}  max|g64| {sc[k]:.3e}  err/noise {ratio:8.3f}")
        assert ratio <= 1.0 + 1e-12          # err = e_o32: 1 / C_TIGHT of the bar
    if c["n"] == 0:
        assert not r64["dW"].any() and not r64["db"].any()
    # dropping the act_super scale of the backward leaves the bar
    if c["act"] > 0 and c["n"] > 0:
        bad = r64["d_feat"].copy()
        bad[:, 1:] /= 1 + 2e-3
        assert OR.head_ratio(bad, r64["d_feat"], e["d_feat"], sc["d_feat"])[1] > 10 * OR.C_TIGHT
    if c["sat"]:
        lo, hi = OR.head_end_values(c["act"])
        assert len(c["sat"]) == 12 and set(c["sat"].values()) == set(OR.SAT_SIGNS)
        z = c["feat"][:c["n"], 1:129].astype(np.float64) @ c["w"].astype(np.float64).T + c["b"]
        for r, sg in c["sat"].items():
            assert np.allclose(z[r], OR.SAT_LOGIT * np.array(sg), atol=1e-3)
            assert np.array_equal(r32["out"][r, 1:], np.where(np.array(sg) > 0, hi, lo).astype(F32))
            assert not r32["d_feat"][r, 1:].any() and np.isfinite(r32["out"][r]).all()
        assert np.isfinite(r32["dW"]).all()
