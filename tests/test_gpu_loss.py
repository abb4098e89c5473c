"""The objective on the device (pointnerf_amd.losses, pnr_color_loss_* /
pnr_sparse_loss_*) against tests/loss_ref.py, the torch restatement of the
reference's compute_losses: float64 is the truth, float32 the yardstick.

Rule (loss_ref.within): an error of at most 4 x the fp32
restatement's own error vs fp64 plus one fp32 ulp of the value (for a gradient,
of the tensor's largest entry); every ray and every point is compared.
Measured on MI355X: the kernels sum in fp64 and round once, so every value and
gradient sits within that one ulp (largest err / allowed per case: DESIGN.md
"Objective")."""
import numpy as np
import pytest
import torch

import loss_ref as LR
from formula import UPSTREAM_SHAPES, formula_params
from scenes import scene
from test_gpu_train_contract import _inputs, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _collect_models():
    """A training-mode model sits in a reference cycle (last_train_aux's lazy
    entries hold it), so its grid handle waits for the collector: free this
    module's models when it is done instead of leaving them to a later test."""
    yield
    import gc
    from pointnerf_amd import querier as Q
    _STEP.clear()
    gc.collect()
    Q.release_deferred()

ALL4 = ("coarse_raycolor", "ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor",
        "ray_depth_masked_coarse_raycolor")
UPSTREAM = (0.7, 1.3, 0.25, 2.0)     # d loss / d item: all four kinds at once, none of them 1
LEGO_ITEMS = ["ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor"]


def _colour_case(R, layout, masks, cuda, seed):
    """x (requires grad, maybe a [:, :3] view of [R,128]), gt, ray_mask, extra."""
    g = torch.Generator().manual_seed(seed)
    C = 128 if layout == "c128" else 3
    base = torch.rand((R, 128 if layout == "c3_of_128" else C), generator=g).to(cuda)
    gt = torch.rand((1, R, C), generator=g).to(cuda)
    if masks == "hit":
        rm = torch.ones(R, dtype=torch.int8)
    elif masks == "miss":
        rm = torch.zeros(R, dtype=torch.int8)
    else:
        rm = (torch.rand(R, generator=g) < 0.4).to(torch.int8)
    extra = torch.zeros(R, dtype=torch.uint8) if masks == "mixed_empty_extra" else \
        (torch.rand(R, generator=g) < 0.5).to(torch.uint8)
    return base, gt, rm.to(cuda), extra.to(cuda), C


def _ref_items(x, gt, rm, extra, dtype):
    """The four items by the restatement in `dtype` (leaf x) -> (values, x).  An
    empty ray_depth_masked_ set is 0 here by definition (NaN in the reference)."""
    xl = x.detach().to(dtype).requires_grad_(True)
    out = {"coarse_raycolor": xl[None], "ray_mask": rm[None]}
    vals = []
    for name in ALL4:
        if name.startswith("ray_depth_masked") and int(extra.sum()) == 0:
            vals.append((xl * 0).sum())
        else:
            vals.append(LR.color_item(name, out, gt.to(dtype), extra).to(dtype))
    return torch.stack(vals), xl


@pytest.mark.parametrize("layout", ["c3", "c128", "c3_of_128"])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 257, 3600])
def test_color_losses_value_and_gradient(cuda, R, layout):
    from pointnerf_amd.losses import color_losses
    worst = 0.0
    for mi, masks in enumerate(("hit", "miss", "mixed", "mixed_empty_extra")):
        base, gt, rm, extra, C = _colour_case(R, layout, masks, cuda, 100 * R + mi)
        base.requires_grad_(True)
        x = base[:, :3] if layout == "c3_of_128" else base
        if layout == "c3_of_128":
            assert x.stride(0) == 128
        v, counts = color_losses(x[None], gt, rm[None], extra)
        assert v.shape == (4,) and v.dtype == torch.float32 and counts.dtype == torch.int64
        n_hit, n_miss, n_ex = int((rm > 0).sum()), int((rm == 0).sum()), int((extra > 0).sum())
        assert counts.tolist() == [R, n_hit, n_miss, n_ex]
        up = torch.tensor(UPSTREAM, device=cuda)
        (v * up).sum().backward()
        got_g = base.grad[:, :3] if layout == "c3_of_128" else base.grad
        if layout == "c3_of_128":
            assert not base.grad[:, 3:].any()      # the view's backward touches its own columns only
        r64, x64 = _ref_items(x, gt, rm, extra, torch.float64)
        r32, x32 = _ref_items(x, gt, rm, extra, torch.float32)
        (r64 * up.double()).sum().backward()
        (r32 * up).sum().backward()
        tag = f"R={R} {layout} {masks}"
        for k, name in enumerate(ALL4):
            worst = max(worst, LR.within(v[k], r64[k], r32[k], f"{tag} {name}"))
        worst = max(worst, LR.within(got_g, x64.grad, x32.grad, f"{tag} d x"))
        assert torch.isfinite(v).all() and torch.isfinite(got_g).all()
        # empty sets: exactly 0, and no gradient from them
        for k, n in ((1, n_hit), (2, n_miss), (3, n_ex)):
            if n == 0:
                assert v[k].item() == 0.0, (tag, k)
                xe = x.detach().clone().requires_grad_(True)
                color_losses(xe[None], gt, rm[None], extra)[0][k].backward()
                assert not xe.grad.any() and torch.isfinite(xe.grad).all(), (tag, k)
    print(f"worst ratio R={R} {layout}: {worst:.3f}")


def test_color_losses_single_kind_leaves_other_rows_zero(cuda):
    """Rows outside every requested set get exactly 0."""
    from pointnerf_amd.losses import color_losses
    base, gt, rm, extra, _ = _colour_case(257, "c3", "mixed", cuda, 5)
    x = base.requires_grad_(True)
    color_losses(x, gt, rm, extra)[0][1].backward()      # ray_masked_ only
    assert not x.grad[rm == 0].any() and x.grad[rm > 0].abs().min() > 0
    x.grad = None
    color_losses(x, gt, rm, None)[0][3].backward()       # no extra mask: an empty set
    assert not x.grad.any()


def test_color_losses_repeatable(cuda):
    from pointnerf_amd.losses import color_losses
    for R, layout in ((3600, "c3_of_128"), (257, "c128"), (4096, "c3")):
        base, gt, rm, extra, _ = _colour_case(R, layout, "mixed", cuda, 7)
        runs = []
        for _ in range(2):
            b = base.clone().requires_grad_(True)
            x = b[:, :3] if layout == "c3_of_128" else b
            v, n = color_losses(x, gt, rm, extra)
            (v * torch.tensor(UPSTREAM, device=cuda)).sum().backward()
            runs.append((v.detach().clone(), n.clone(), b.grad.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ through the module
_STEP = {}


def _step_scene():
    """scene(20000, 24 x 24, theta 70): 245 hit and 331 missed rays of 576 (CPU
    oracle), C_out = 3, the lego items with weights 1 1 1, sparse weight 1e-3."""
    if "sc" not in _STEP:
        sc = scene(20000, H=24, W=24, theta=70.0, shading_color_channel_num=3, sparse_loss_weight=1e-3,
                   color_loss_items=list(LEGO_ITEMS), color_loss_weights=[1.0, 1.0, 1.0])
        sc["bg"] = np.array([0.9, 0.8, 1.0], np.float32)
        _STEP["sc"] = sc
        _STEP["params"] = formula_params(UPSTREAM_SHAPES, salt=0.35)
        _STEP["gt"] = torch.rand((1, 24 * 24, 3), generator=torch.Generator().manual_seed(9))
    return _STEP["sc"], _STEP["params"], _STEP["gt"]


def _train_model(cuda, conf=True):
    sc, params, gt = _step_scene()
    m = _model(sc, cuda, params, train=True)
    if not conf:   # the same cloud without a conf table
        from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
        np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                           torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), None)
        m = NeuralPointsRayMarching(sc["opt"], np_, m.aggregator, precision="fp32")
        m.train_precision = "fp32x3"
    m.train()
    return sc, m, gt.to(cuda)


def _gathered_cc(m, conf_leaf):
    """conf_coefficient rebuilt from a leaf of any dtype (renderer._march_aux's lines)."""
    pidx = m.last_train_aux["sample_pidx"]
    cf = conf_leaf.reshape(-1)[pidx.clamp(min=0).long()]
    return cf - (cf - torch.clamp(cf, 1e-4, 1.0)).detach()


def test_sparse_conf_loss_vs_reference_formula(cuda):
    sc, m, _ = _train_model(cuda)
    m(**_inputs(sc, cuda))
    aux = m.last_train_aux
    loss = m.sparse_conf_loss()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * 0.37).backward()
    got_g = m.neural_points.points_conf.grad.clone()
    w, cc = aux["weight"], aux["conf_coefficient"]            # the existing path (reads R'' on the host)
    assert float(w.sum()) > 100 and int((aux["sample_pidx"] < 0).sum()) > 0
    LR.within(loss, LR.sparse_item(w.double(), cc.double()), LR.sparse_item(w, cc), "sparse loss")
    conf = m.neural_points.points_conf.detach()
    leaves = {}
    for dt in (torch.float64, torch.float32):
        leaf = conf.to(dt).clone().requires_grad_(True)
        (LR.sparse_item(w.to(dt), _gathered_cc(m, leaf)) * 0.37).backward()
        leaves[dt] = leaf.grad
    assert int((leaves[torch.float64] != 0).sum()) > 100     # non-trivial: hundreds of points are gathered
    LR.within(got_g, leaves[torch.float64], leaves[torch.float32], "sparse d points_conf")
    # repeatable: the integer atomics commute
    m.neural_points.points_conf.grad = None
    loss2 = m.sparse_conf_loss()
    (loss2 * 0.37).backward()
    assert torch.equal(loss, loss2) and torch.equal(got_g, m.neural_points.points_conf.grad)


def test_sparse_conf_loss_without_conf_table(cuda):
    """conf_coefficient is the constant 1: sum W f(1) / (sum W + 1e-6), no gradient."""
    sc, m, _ = _train_model(cuda, conf=False)
    m(**_inputs(sc, cuda))
    loss = m.sparse_conf_loss()
    assert not loss.requires_grad
    w = m.last_train_aux["weight"]
    one = torch.ones((), device=cuda)
    LR.within(loss, LR.sparse_item(w.double(), one.double()), LR.sparse_item(w, one), "sparse loss, no conf")
    assert torch.equal(loss, m.sparse_conf_loss())


def _grads(m, bg):
    return {"points_conf": m.neural_points.points_conf.grad.clone(), "bg_color": bg.grad.clone(),
            "block1.0.weight": dict(m.aggregator.named_parameters())["block1.0.weight"].grad.clone()}


def test_step_matches_reference_objective(cuda):
    """model(...) in training mode, then RenderLoss against tests/loss_ref.py on
    the same output (fp32 torch autograd = the yardstick, fp64 = the truth):
    loss_total, every item and the gradients that reach the point table, the
    background and the aggregator."""
    from pointnerf_amd.losses import RenderLoss
    sc, m, gt = _train_model(cuda)
    opt = sc["opt"]
    res, first = {}, None
    for variant in ("native", torch.float64, torch.float32):
        m.zero_grad(set_to_none=True)
        bg = torch.from_numpy(sc["bg"]).to(cuda).requires_grad_(True)
        out = m(**_inputs(sc, cuda, bg=bg))
        if first is None:
            first = out["coarse_raycolor"].detach().clone()
            mask = out["ray_mask"]
            assert (int((mask > 0).sum()), int((mask == 0).sum())) == (245, 331)
        assert torch.equal(out["coarse_raycolor"].detach(), first)       # the same output every time
        leaf = None
        if variant == "native":
            total, items = RenderLoss(opt)(out, gt, model=m)
        else:
            ref_out = LR.cast(out, variant)
            if variant == torch.float64:
                # the truth is fp64 from the conf table on: through the dict entry the gather's
                # backward would add ~155 000 fp32 terms into point 0 (the empty slots)
                leaf = m.neural_points.points_conf.detach().double().requires_grad_(True)
                ref_out["conf_coefficient"] = _gathered_cc(m, leaf)
                assert torch.equal(ref_out["conf_coefficient"].float(), out["conf_coefficient"])
            total, items = LR.compute_losses(opt, ref_out, gt.to(variant))
        total.backward()
        grads = _grads(m, bg)
        if leaf is not None:   # the render's share (fp32 kernels) + the zero-one and sparse shares (fp64)
            grads["points_conf"] = grads["points_conf"].double() + leaf.grad
        res[variant] = (total.detach(), {k: v.detach() for k, v in items.items()}, grads)
    nat, r64, r32 = res["native"], res[torch.float64], res[torch.float32]
    LR.within(nat[0], r64[0], r32[0], "loss_total")
    names = ["loss_" + n for n in LEGO_ITEMS] + ["loss_conf_coefficient", "loss_sparse"]
    assert sorted(r64[1]) == sorted(names)
    for k in names:
        LR.within(nat[1][k], r64[1][k], r32[1][k], k)
        assert float(r64[1][k].abs()) > 0
    for k in LEGO_ITEMS:
        assert nat[1]["psnr_" + k].is_cuda
        LR.within(nat[1]["psnr_" + k], LR.mse2psnr(r64[1]["loss_" + k]), LR.mse2psnr(r32[1]["loss_" + k]), "psnr_" + k)
    for k in nat[2]:
        assert float(r64[2][k].abs().max()) > 0
        LR.within(nat[2][k], r64[2][k], r32[2][k], "d " + k)


def test_objective_reads_nothing_on_the_host(cuda, capsys):
    from pointnerf_amd.losses import RenderLoss
    sc, m, gt = _train_model(cuda)
    rl = RenderLoss(sc["opt"])
    out = m(**_inputs(sc, cuda))
    rl(out, gt, model=m)          # first call: the cached weight vector, library scratch
    reads = m.train_count_reads
    out = m(**_inputs(sc, cuda))
    ran_debug = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        ran_debug = True
    except Exception as e:    # this torch build has no sync debug mode on ROCm
        print("set_sync_debug_mode unavailable:", repr(e))
    try:
        total, _ = rl(out, gt, model=m)
    finally:
        if ran_debug:
            torch.cuda.set_sync_debug_mode("default")
    m.zero_one_conf_loss()
    m.sparse_conf_loss()
    total.backward()
    assert m.train_count_reads == reads
    with capsys.disabled():
        print(f"\n[no-host-read] train_count_reads check ran; sync debug mode 'error' around RenderLoss: "
              f"{'ran' if ran_debug else 'not available'}")


def test_frame_metrics_on_a_frame(cuda):
    from pointnerf_amd.losses import frame_metrics
    g = torch.Generator().manual_seed(3)
    R = 64 * 64
    out = {"coarse_raycolor": torch.rand((1, R, 3), generator=g).to(cuda),
           "ray_mask": (torch.rand((1, R), generator=g) < 0.6).to(torch.int8).to(cuda)}
    gt = torch.rand((1, R, 3), generator=g).to(cuda)
    items = ["coarse_raycolor", "ray_miss_coarse_raycolor", "ray_masked_coarse_raycolor"]   # lego.sh:154
    got = frame_metrics(out, gt, items)
    assert sorted(got) == sorted(["loss_" + n for n in items] + ["psnr_" + n for n in items])
    for n in items:
        r64 = LR.color_item(n, LR.cast(out, torch.float64), gt.double())
        r32 = LR.color_item(n, out, gt)
        assert got["psnr_" + n].is_cuda and got["loss_" + n].is_cuda and not got["loss_" + n].requires_grad
        LR.within(got["loss_" + n], r64, r32, "frame " + n)
        LR.within(got["psnr_" + n], LR.mse2psnr(r64), LR.mse2psnr(r32), "frame psnr " + n)
