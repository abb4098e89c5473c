"""The objective's host side (no GPU): tests/loss_ref.py against hand-computed
values, RenderLoss's option handling and refusals, and the argument checks of
pnr_color_loss_* / pnr_sparse_loss_* (PNR_EINVAL before any launch)."""
import math
import os
import subprocess
from types import SimpleNamespace

import pytest
import torch

import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pointnerf_amd", "libpnr.so")


def _four_rays(dtype=torch.float64):
    # squared errors per ray: 1, 4, 9, 3 (gt = 0); rays 0 and 2 hit, 1 and 3 miss
    x = torch.tensor([[[1., 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 1]]], dtype=dtype)
    out = {"coarse_raycolor": x, "ray_mask": torch.tensor([[1, 0, 1, 0]], dtype=torch.int8)}
    return out, torch.zeros((1, 4, 3), dtype=dtype)


def test_restatement_on_four_rays_by_hand():
    out, gt = _four_rays()
    assert LR.color_item("coarse_raycolor", out, gt).item() == pytest.approx(17 / 12, rel=1e-14)
    assert LR.color_item("ray_masked_coarse_raycolor", out, gt).item() == pytest.approx(10 / 6, rel=1e-14)
    assert LR.color_item("ray_miss_coarse_raycolor", out, gt).item() == pytest.approx(7 / 6 * 2, rel=1e-14)
    dm = torch.tensor([0, 0, 0, 1])
    assert LR.color_item("ray_depth_masked_coarse_raycolor", out, gt, dm).item() == pytest.approx(1.0, rel=1e-14)
    assert math.isnan(LR.color_item("ray_depth_masked_coarse_raycolor", out, gt, torch.zeros(4)).item())
    # the Python branches on an empty selection (:547-550, :559-562)
    all_miss = dict(out, ray_mask=torch.zeros((1, 4), dtype=torch.int8))
    assert LR.color_item("ray_masked_coarse_raycolor", all_miss, gt).item() == 0.0
    assert LR.color_item("ray_miss_coarse_raycolor", all_miss, gt).item() == pytest.approx(17 / 12 * 4, rel=1e-14)
    all_hit = dict(out, ray_mask=torch.ones((1, 4), dtype=torch.int8))
    assert LR.color_item("ray_miss_coarse_raycolor", all_hit, gt).item() == 0.0
    zo = LR.zero_one_item(torch.tensor([0.5, 0.0005], dtype=torch.float64), 1e-3)
    assert zo.item() == pytest.approx((2 * math.log(0.5) + math.log(1e-3) + math.log(1 - 1e-3)) / 2, rel=1e-14)
    sp = LR.sparse_item(torch.tensor([0.25, 0.75], dtype=torch.float64), torch.tensor([1.0, 0.5], dtype=torch.float64))
    assert sp.item() == pytest.approx((0.25 * (1 - math.exp(-2)) + 0.75 * (1 - math.exp(-1))) / (1 + 1e-6), rel=1e-14)
    opt = SimpleNamespace(color_loss_items=["ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor"],
                          color_loss_weights=[2.0], zero_one_loss_items=[], sparse_loss_weight=0)
    total, d = LR.compute_losses(opt, out, gt)
    assert total.item() == pytest.approx(2 * (10 / 6 + 7 / 3 + 17 / 12) + 3e-6, rel=1e-14)
    assert sorted(d) == ["loss_coarse_raycolor", "loss_ray_masked_coarse_raycolor", "loss_ray_miss_coarse_raycolor"]
    assert LR.mse2psnr(torch.tensor(0.01, dtype=torch.float64)).item() == pytest.approx(20.0, rel=1e-12)


def _torch_color_losses(x, gt, ray_mask, extra_mask=None):
    """color_losses' contract in torch ops (a CPU stand-in for the kernel)."""
    x2, g2 = x.reshape(-1, x.shape[-1]), gt.reshape(-1, gt.shape[-1])
    C = x2.shape[1]
    d2 = ((x2 - g2) ** 2).sum(1)
    rm = ray_mask.reshape(-1)
    em = torch.zeros_like(rm, dtype=torch.bool) if extra_mask is None else extra_mask.reshape(-1) > 0
    sets = (torch.ones_like(rm, dtype=torch.bool), rm > 0, rm == 0, em)
    n = torch.stack([s.sum() for s in sets])
    vals = []
    for k, s in enumerate(sets):
        den = (1 if k == 2 else int(n[k])) * C
        vals.append(d2[s].sum() / den if int(n[k]) else d2.sum() * 0)
    return torch.stack(vals), n


def _opt(**kw):
    base = dict(color_loss_items=["ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor"],
                color_loss_weights=[1.0, 0.0, 0.0], zero_one_loss_items=[], zero_one_loss_weights=[1e-4],
                zero_epsilon=1e-3, sparse_loss_weight=0, depth_loss_items=[], bg_loss_items=[], l2_size_loss_items=[])
    if "color_loss_items" in kw and "color_loss_weights" not in kw:
        base["color_loss_weights"] = [1.0]
    base.update(kw)
    return SimpleNamespace(**base)


def test_render_loss_weights_and_epsilon(monkeypatch):
    from pointnerf_amd import losses
    monkeypatch.setattr(losses, "color_losses", _torch_color_losses)
    out, gt = _four_rays(torch.float32)
    rl = losses.RenderLoss(_opt(color_loss_weights=[2.0]))           # one weight for every item (:232-234)
    assert rl.color_weights == [2.0, 2.0, 2.0]
    total, d = rl(out, gt)
    assert total.dtype == torch.float32
    assert total.item() == pytest.approx(2 * (10 / 6 + 7 / 3 + 17 / 12) + 3e-6, rel=3e-7)   # + 1e-6 per item (:603)
    assert d["loss_ray_miss_coarse_raycolor"].item() == pytest.approx(7 / 3, rel=3e-7)
    assert d["psnr_coarse_raycolor"].item() == pytest.approx(-10 * math.log10(17 / 12), rel=1e-5)
    # zero weights still add their 1e-6; the zero-one and sparse terms from the dict entries
    out["conf_coefficient"] = torch.tensor([[[[0.5, 0.0005]]]])
    out["weight"] = torch.tensor([[[[0.25, 0.75]]]])
    rl = losses.RenderLoss(_opt(color_loss_weights=[0.0, 0.0, 0.0], zero_one_loss_items=["conf_coefficient"],
                                zero_one_loss_weights=[0.5], sparse_loss_weight=0.25))
    total, d = rl(out, gt)
    zo = (2 * math.log(0.5) + math.log(1e-3) + math.log(1 - 1e-3)) / 2
    sp = (0.25 * (1 - math.exp(-2 * 0.5)) + 0.75 * (1 - math.exp(-2 * 0.0005))) / (1 + 1e-6)
    assert d["loss_conf_coefficient"].item() == pytest.approx(zo, rel=1e-6)
    assert d["loss_sparse"].item() == pytest.approx(sp, rel=1e-6)
    assert total.item() == pytest.approx(3e-6 + 0.5 * zo + 0.25 * sp, rel=1e-6)
    ref_total, _ = LR.compute_losses(rl.opt, out, gt)
    assert total.item() == pytest.approx(ref_total.item(), rel=1e-6)
    with pytest.raises(losses.L.PnrError, match="3 items"):
        losses.RenderLoss(_opt(color_loss_weights=[1.0, 2.0]))


def test_render_loss_refusals(monkeypatch):
    from pointnerf_amd import losses
    from pointnerf_amd._lib import PnrError
    monkeypatch.setattr(losses, "color_losses", _torch_color_losses)
    out, gt = _four_rays(torch.float32)
    with pytest.raises(PnrError, match="unknown kind"):
        losses.RenderLoss(_opt(color_loss_items=["ray_edge_coarse_raycolor"]))
    for group in ("depth_loss_items", "bg_loss_items", "l2_size_loss_items"):
        with pytest.raises(PnrError, match=group):
            losses.RenderLoss(_opt(**{group: ["coarse_depth"]}))
    with pytest.raises(PnrError, match="no 'final_coarse_raycolor'"):
        losses.RenderLoss(_opt(color_loss_items=["final_coarse_raycolor"]))(out, gt)
    with pytest.raises(PnrError, match="no 'ray_mask'"):
        losses.RenderLoss(_opt())({"coarse_raycolor": out["coarse_raycolor"]}, gt)
    with pytest.raises(PnrError, match="no 'weight'"):
        losses.RenderLoss(_opt(sparse_loss_weight=1e-3))(out, gt)
    with pytest.raises(PnrError, match="no 'conf_coefficient'"):
        losses.RenderLoss(_opt(zero_one_loss_items=["conf_coefficient"]))(out, gt)
    wide = dict(out, coarse_raycolor=torch.zeros((1, 4, 128)))
    with pytest.raises(PnrError, match="128 channels, gt_image 3"):
        losses.RenderLoss(_opt())(wide, gt)
    with pytest.raises(PnrError, match="ray_depth_mask"):
        losses.RenderLoss(_opt(color_loss_items=["ray_depth_masked_coarse_raycolor"]))(out, gt)
    with pytest.raises(PnrError, match="128 channels"):
        losses.frame_metrics(wide, gt, ["coarse_raycolor"])


def test_lego_options_carry_the_objective():
    from pointnerf_amd.options import lego_opt
    o = lego_opt()
    assert o.color_loss_items == ["ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor"]
    assert o.color_loss_weights == [1.0, 0.0, 0.0]
    assert o.zero_one_loss_weights == [0.0001] and o.zero_epsilon == 1e-3
    import pointnerf_amd
    assert pointnerf_amd.RenderLoss is pointnerf_amd.losses.RenderLoss
    assert callable(pointnerf_amd.color_losses) and callable(pointnerf_amd.frame_metrics)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "pointnerf_amd/libpnr.so"])
    from pointnerf_amd import _lib as L
    return L


def test_loss_entry_points_validate_on_the_host(lib):
    """Bad arguments return PNR_EINVAL before any launch: the fake pointers
    are never dereferenced and no GPU is needed."""
    L = lib
    so = L.lib()
    p = L.c_void_p(0x1000)
    nb = L.c_size_t(0)
    assert so.pnr_color_loss_scratch_bytes(L.ctypes.byref(nb)) == L.PNR_OK and nb.value > 0
    assert so.pnr_color_loss_scratch_bytes(None) == L.PNR_EINVAL
    fwd = lambda x=p, ldx=3, gt=p, ldgt=3, rm=p, R=10, C=3, out=p, cnt=p, scr=p, n=None: so.pnr_color_loss_fwd(  # noqa: E731
        x, ldx, gt, ldgt, rm, None, R, C, out, cnt, scr, nb.value if n is None else n, None)
    assert fwd(x=None) == L.PNR_EINVAL and b"null" in so.pnr_last_error()
    assert fwd(gt=None) == L.PNR_EINVAL
    assert fwd(rm=None) == L.PNR_EINVAL
    assert fwd(out=None) == L.PNR_EINVAL
    assert fwd(cnt=None) == L.PNR_EINVAL
    assert fwd(scr=None) == L.PNR_EINVAL
    assert fwd(C=129, ldx=129, ldgt=129) == L.PNR_EINVAL and b"C=129" in so.pnr_last_error()
    assert fwd(C=0) == L.PNR_EINVAL
    assert fwd(R=-1) == L.PNR_EINVAL and b"R < 0" in so.pnr_last_error()
    assert fwd(ldx=2) == L.PNR_EINVAL and b"stride" in so.pnr_last_error()
    assert fwd(n=8) == L.PNR_EINVAL and b"scratch too small" in so.pnr_last_error()
    bwd = lambda x=p, R=10, C=3, cnt=p, g=p, d=p, ldd=3: so.pnr_color_loss_bwd(  # noqa: E731
        x, 3 if C <= 3 else C, p, 3 if C <= 3 else C, p, None, R, C, cnt, g, d, ldd, None)
    assert bwd(x=None) == L.PNR_EINVAL
    assert bwd(cnt=None) == L.PNR_EINVAL
    assert bwd(g=None) == L.PNR_EINVAL
    assert bwd(d=None) == L.PNR_EINVAL
    assert bwd(C=129) == L.PNR_EINVAL
    assert bwd(R=-5) == L.PNR_EINVAL
    assert bwd(ldd=2) == L.PNR_EINVAL
    qp = L.QueryParams()
    qp.SR, qp.K = 80, 8
    qb = L.QueryBufs()
    assert so.pnr_sparse_loss_scratch_bytes(L.ctypes.byref(nb)) == L.PNR_OK and nb.value > 0
    sp = lambda q=L.ctypes.byref(qp), b=L.ctypes.byref(qb), R=10, xyz=p, N=100, wf=p, out=p, st=p, scr=p: \
        so.pnr_sparse_loss_fwd(q, b, R, xyz, None, N, wf, out, st, scr, nb.value, None)  # noqa: E731
    assert sp(q=None) == L.PNR_EINVAL
    assert sp(b=None) == L.PNR_EINVAL
    assert sp(xyz=None) == L.PNR_EINVAL
    assert sp(wf=None) == L.PNR_EINVAL
    assert sp(out=None) == L.PNR_EINVAL
    assert sp(R=-1) == L.PNR_EINVAL
    assert sp(N=0) == L.PNR_EINVAL
    assert sp() == L.PNR_EINVAL and b"query buffers missing" in so.pnr_last_error()   # an empty pnr_query_bufs
    assert sp(R=1 << 20) == L.PNR_EINVAL and b"fixed-point" in so.pnr_last_error()
    qp.K = 17
    assert sp() == L.PNR_EINVAL and b"K=17" in so.pnr_last_error()
    assert so.pnr_sparse_loss_bwd(None, p, 100, p, p, p, None) == L.PNR_EINVAL
    assert so.pnr_sparse_loss_bwd(p, None, 100, p, p, p, None) == L.PNR_EINVAL
    assert so.pnr_sparse_loss_bwd(p, p, 0, p, p, p, None) == L.PNR_EINVAL
