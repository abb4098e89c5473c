"""Composite and the full fused render vs the oracle / reference golden."""
import os

import numpy as np
import pytest
import torch

from formula import formula_params
from oracle import oracle as O
from scenes import oracle_points, scene

pytestmark = pytest.mark.gpu


def test_ray_march_vs_reference_golden(golden_dir, cuda):
    from pointnerf_amd.ray_march import alpha_blend, radiance_render, ray_march
    g = np.load(os.path.join(golden_dir, "raymarch.npz"), allow_pickle=False)
    t = {k: torch.from_numpy(g[k]).to(cuda) for k in ("ray_dist", "ray_valid", "ray_features", "bg_color")}
    out = ray_march(t["ray_dist"], t["ray_valid"], t["ray_features"], radiance_render, alpha_blend, t["bg_color"])
    names = ["ray_color", "point_color", "opacity", "acc_transmission", "blend_weight",
             "background_transmission", "background_blend_weight"]
    for n, o in zip(names, out):
        np.testing.assert_allclose(o.cpu().numpy(), g[n], atol=2e-5, rtol=1e-5, err_msg=n)


def _renderer(sc, cuda, params, chunk=None):
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.renderer import NeuralPoints, NeuralPointsRayMarching
    agg = PointAggregator(sc["opt"]).to(cuda)
    agg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    np_ = NeuralPoints(sc["opt"], cuda, torch.from_numpy(sc["xyz"]), torch.from_numpy(sc["emb"]),
                       torch.from_numpy(sc["color"]), torch.from_numpy(sc["dir"]), torch.from_numpy(sc["conf"]))
    return NeuralPointsRayMarching(sc["opt"], np_, agg.eval(), chunk_rays=chunk, precision="fp32")


def _forward(m, sc, cuda):
    with torch.no_grad():
        return m(campos=torch.from_numpy(sc["campos"]).to(cuda)[None],
                 raydir=torch.from_numpy(sc["raydir"]).to(cuda)[None],
                 bg_color=torch.from_numpy(sc["bg"]).to(cuda),
                 camrotc2w=torch.from_numpy(sc["camrot"]).to(cuda)[None],
                 near=torch.tensor([[2.0]], device=cuda), far=torch.tensor([[6.0]], device=cuda))


@pytest.mark.parametrize("theta", [30.0, 200.0])
def test_render_vs_oracle(cuda, theta):
    sc = scene(30000, H=48, W=48, theta=theta, default_conf=None)
    params = formula_params(salt=0.1)
    out = _forward(_renderer(sc, cuda, params), sc, cuda)
    ref = O.render(sc["opt"], oracle_points(sc), params, sc["campos"], sc["camrot"], sc["raydir"], sc["bg"])
    assert np.array_equal(out["ray_mask"].cpu().numpy()[0], ref["ray_mask"])
    assert ref["ray_mask"].sum() > 200
    np.testing.assert_allclose(out["coarse_raycolor"].cpu().numpy()[0], ref["coarse_raycolor"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["coarse_point_opacity"].cpu().numpy()[0], ref["coarse_point_opacity"],
                               atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(out["coarse_is_background"].cpu().numpy()[0], ref["coarse_is_background"],
                               atol=2e-4, rtol=1e-4)
    np.testing.assert_array_equal(out["queried_shading"].cpu().numpy()[0], ref["queried_shading"])
    # image-level criterion of SURVEY 8(d): PSNR(build vs oracle) >= 60 dB
    a, b = out["coarse_raycolor"].cpu().numpy()[0], ref["coarse_raycolor"]
    mse = float(np.mean((a - b) ** 2))
    peak = float(np.abs(b).max())
    assert 10 * np.log10(peak ** 2 / max(mse, 1e-30)) >= 60.0


def test_chunked_equals_whole_and_deterministic(cuda):
    sc = scene(20000, H=40, W=40)
    params = formula_params(salt=0.2)
    a = _forward(_renderer(sc, cuda, params), sc, cuda)
    b = _forward(_renderer(sc, cuda, params, chunk=333), sc, cuda)
    c = _forward(_renderer(sc, cuda, params), sc, cuda)
    for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "ray_mask"):
        assert torch.equal(a[k], c[k]), k          # bitwise repeatable (no float atomics)
        assert torch.allclose(a[k].float(), b[k].float(), atol=1e-6), k


def test_all_background(cuda):
    sc = scene(5000, H=8, W=8)
    sc["raydir"] = -sc["raydir"]
    out = _forward(_renderer(sc, cuda, formula_params()), sc, cuda)
    assert int(out["ray_mask"].sum()) == 0
    bg = torch.from_numpy(sc["bg"]).to(cuda)
    assert torch.equal(out["coarse_raycolor"][0], bg.expand(64, 128))
    assert torch.all(out["coarse_is_background"] == 1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reuse_p1_across_batches(cuda, precision):
    """render_rays(reuse_p1=True) (the partial frames of one multi-GPU step)
    equals a fresh computation bitwise, and an in-place change of block1.0 or
    the embedding invalidates the reused per-point half."""
    sc = scene(20000, H=40, W=40, theta=30.0)
    sc2 = scene(20000, H=40, W=40, theta=200.0)
    params = formula_params(salt=0.3)
    m = _renderer(sc, cuda, params)
    m.precision = precision
    cp, cr, bg = (torch.from_numpy(sc[k]).to(cuda) for k in ("campos", "camrot", "bg"))
    cp2, cr2 = torch.from_numpy(sc2["campos"]).to(cuda), torch.from_numpy(sc2["camrot"]).to(cuda)
    rd = torch.from_numpy(sc["raydir"]).to(cuda)
    rd2 = torch.from_numpy(sc2["raydir"]).to(cuda)
    fresh = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg)[0]
    m.render_rays(cp, cr, rd[1::2].contiguous(), 2.0, 6.0, bg)
    reused = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg, reuse_p1=True)[0]
    assert torch.equal(fresh, reused)
    with torch.no_grad():
        m.aggregator.block1[0].weight.mul_(0.5)
    stale_check = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg, reuse_p1=True)[0]
    new = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg)[0]
    assert torch.equal(stale_check, new) and not torch.equal(new, fresh)
    with torch.no_grad():
        m.neural_points.points_embeding.add_(0.25)
    stale_check = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg, reuse_p1=True)[0]
    new2 = m.render_rays(cp2, cr2, rd2[::2].contiguous(), 2.0, 6.0, bg)[0]
    assert torch.equal(stale_check, new2) and not torch.equal(new2, new)


def test_train_render_refuses_bg_channels(cuda):
    """render_rays_train refuses a bg_color of neither 1 nor C channels on the
    host, before the query (no grid is built, no query buffers are kept) -- the
    composite kernel would read C floats from it."""
    from pointnerf_amd._lib import PnrError
    sc = scene(5000, H=8, W=8)
    m = _renderer(sc, cuda, formula_params()).train()
    cp, cr, rd = (torch.from_numpy(sc[k]).to(cuda) for k in ("campos", "camrot", "raydir"))
    with pytest.raises(PnrError, match="bg_color must have 1 or 128 channels"):
        m.render_rays_train(cp, cr, rd, 2.0, 6.0, torch.zeros(2, device=cuda))
    assert m.neural_points.querier.grid.key is None and m._train_conf_src is None
