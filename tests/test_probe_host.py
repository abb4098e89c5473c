"""Point growing on the host (no GPU): the per-frame selection and the frame loop
of pointnerf_amd.probe (run/train_ft.py:420-543) on hand-made maps, and
pnr_probe's argument validation."""
import os
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pointnerf_amd", "libpnr.so")
H, W = 6, 7


def _maps():
    """6x7 maps: every ray hits with maximum opacity 0.9 and gt == render == bg,
    except the pixels the tests plant."""
    bg = torch.tensor([0.2, 0.4, 0.6])
    gt = bg.expand(H, W, 3).clone()
    maps = dict(ray_mask=torch.ones(H, W, 1), ray_max_shading_opacity=torch.full((H, W, 1), 0.9),
                ray_max_far_dist=torch.full((H, W, 1), 0.001), coarse_raycolor=gt.clone())

    def miss(y, x):
        maps["ray_mask"][y, x] = 0
        gt[y, x] += 0.3
        maps["coarse_raycolor"][y, x] = bg

    miss(0, 0)                                   # corner: the border clamp
    miss(3, 3)                                   # interior
    maps["ray_mask"][5, 6] = 0                   # true background (gt == bg): no miss
    maps["ray_max_shading_opacity"][2, 3] = 0.5  # a neighbour of (3, 3) below opacity_thresh
    maps["ray_max_far_dist"][0, 5] = 0.02        # far ray, render == gt
    maps["ray_max_far_dist"][5, 0] = 0.02        # far ray, but the render is off: not grown
    maps["coarse_raycolor"][5, 0] += 0.5
    return maps, gt, bg


def _mask(pixels):
    m = torch.zeros(H, W, dtype=torch.bool)
    for y, x in pixels:
        m[y, x] = True
    return m


CORNER = [(0, 1), (1, 0), (1, 1)]
INTERIOR = [(y, x) for y in (2, 3, 4) for x in (2, 3, 4) if (y, x) not in ((3, 3), (2, 3))]


def test_select_grow_candidates_dilation_border_and_threshold():
    from pointnerf_amd.probe import select_grow_candidates
    maps, gt, bg = _maps()
    sel = select_grow_candidates(maps, gt, bg, None, far_thresh=-1.0, opacity_thresh=0.7)
    assert sel.dtype == torch.bool and sel.shape == (H, W)
    # nothing wraps to the last row / column from the corner pixel, the miss pixels
    # themselves (ray_mask 0) and the low-opacity neighbour stay out
    assert torch.equal(sel, _mask(CORNER + INTERIOR))
    # a lower threshold lets the 0.5 neighbour in
    sel = select_grow_candidates(maps, gt, bg, None, far_thresh=-1.0, opacity_thresh=0.4)
    assert torch.equal(sel, _mask(CORNER + INTERIOR + [(2, 3)]))


def test_select_grow_candidates_far_rays_and_edge_mask():
    from pointnerf_amd.probe import select_grow_candidates
    maps, gt, bg = _maps()
    sel = select_grow_candidates(maps, gt, bg, None, far_thresh=0.01, opacity_thresh=0.7)
    assert torch.equal(sel, _mask(CORNER + INTERIOR + [(0, 5)]))
    sel = select_grow_candidates(maps, gt, bg, None, far_thresh=0.05, opacity_thresh=0.7)
    assert torch.equal(sel, _mask(CORNER + INTERIOR))
    # (3, 3) was not rendered: it is no miss ray
    edge = torch.ones(H, W, dtype=torch.bool)
    edge[3, 3] = False
    sel = select_grow_candidates(maps, gt, bg, edge, far_thresh=-1.0, opacity_thresh=0.7)
    assert torch.equal(sel, _mask(CORNER))
    # far term with a feature render that cannot be compared with the RGB ground truth
    maps["coarse_raycolor"] = torch.zeros(H, W, 128)
    from pointnerf_amd._lib import PnrError
    with pytest.raises(PnrError):
        select_grow_candidates(maps, gt, bg, None, far_thresh=0.01, opacity_thresh=0.7)


class _Stub:
    """probe_rays returns canned outputs, one per frame, and records the options
    it was called under."""

    def __init__(self, outs):
        self.opt = SimpleNamespace(prob=0, query_size=[3, 3, 3], kernel_size=[3, 3, 3])
        self.outs = list(outs)
        self.seen = []

    def probe_rays(self, campos, camrot, raydir, near, far, bg_color):
        self.seen.append((self.opt.prob, list(self.opt.query_size), near, far))
        return self.outs[len(self.seen) - 1]


def _frame_out(R, miss, base, color=True):
    """R rays, ray `miss` misses; per-ray values base + ray index."""
    ar = torch.arange(R, dtype=torch.float32)
    mask = torch.ones(1, R, dtype=torch.int8)
    mask[0, miss] = 0
    out = dict(coarse_raycolor=torch.zeros(1, R, 3), ray_mask=mask,
               ray_max_sample_loc_w=(base + ar)[None, :, None].repeat(1, 1, 3),
               ray_max_far_dist=torch.zeros(1, R, 1), ray_max_shading_opacity=torch.full((1, R, 1), 0.9),
               shading_avg_color=(base + 0.25 + ar)[None, :, None].repeat(1, 1, 3) if color else None,
               shading_avg_dir=None, shading_avg_conf=(1.0 + ar)[None, :, None].clone(),
               shading_avg_embedding=(base + 0.5 + ar)[None, :, None].repeat(1, 1, 32))
    return out


def _frames():
    bg = torch.zeros(3)
    # frame 0: the whole 2x3 frame, ray 4 = pixel (1, 1) misses -> every other pixel is a candidate
    gt0 = torch.zeros(6, 3)
    gt0[4] = 1.0
    f0 = dict(campos=None, camrotc2w=None, raydir=torch.zeros(6, 3), gt_image=gt0, bg_color=bg, pixel_idx=None,
              h=2, w=3)
    # frame 1: 4 of the 3x3 pixels, rays in the order (x, y) = (2,2), (0,0), (1,1), (2,1); ray 1 = pixel
    # (0, 0) misses -> of the rendered pixels only (1, 1) is within its 3x3; map order puts it first
    gt1 = torch.zeros(4, 3)
    gt1[1] = 1.0
    px = torch.tensor([[2, 2], [0, 0], [1, 1], [2, 1]])
    f1 = dict(campos=None, camrotc2w=None, raydir=torch.zeros(4, 3), gt_image=gt1, bg_color=bg, pixel_idx=px,
              h=3, w=3, near=0.5, far=9.0)
    return [f0, f1]


def _opt(**over):
    o = dict(prob_mul=0.4, far_thresh=-1.0, prob_kernel_size=[3, 3, 3, 5, 5, 5], prob_tiers=[100],
             near_plane=2.0, far_plane=6.0)
    o.update(over)
    return SimpleNamespace(**o)


def test_probe_hole_concatenates_frames_and_restores_options():
    from pointnerf_amd.probe import probe_hole
    stub = _Stub([_frame_out(6, 4, 10.0), _frame_out(4, 1, 100.0)])
    xyz, emb, color, dirs, conf = probe_hole(stub, _frames(), _opt(), opacity_thresh=0.7, test_steps=200)
    # frame 0: rays 0, 1, 2, 3, 5 (row-major pixels); frame 1: ray 2 = pixel (1, 1) only
    want = torch.tensor([10.0, 11.0, 12.0, 13.0, 15.0, 102.0])
    assert torch.equal(xyz, want[:, None].repeat(1, 3))
    assert torch.equal(emb, (want + 0.5)[:, None].repeat(1, 32))
    assert torch.equal(color, (want + 0.25)[:, None].repeat(1, 3))
    assert dirs is None
    # the reference's compounding (train_ft.py:512): frame 0's conf ends at prob_mul^2
    raw = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0, 3.0])[:, None]
    mul = torch.tensor([0.4 * 0.4] * 5 + [0.4])[:, None]
    torch.testing.assert_close(conf, raw * mul, rtol=1e-6, atol=0)
    # rendered with prob = 1 and the tier's query size (200 > prob_tiers[0] -> tier 1), both restored
    assert [s[:2] for s in stub.seen] == [(1, [5, 5, 5])] * 2
    assert stub.seen[0][2:] == (2.0, 6.0) and stub.seen[1][2:] == (0.5, 9.0)
    assert stub.opt.prob == 0 and stub.opt.query_size == [3, 3, 3]


def test_probe_hole_prob_mul_once_and_absent_tables():
    from pointnerf_amd.probe import probe_hole
    stub = _Stub([_frame_out(6, 4, 10.0, color=False), _frame_out(4, 1, 100.0, color=False)])
    opt = _opt(prob_kernel_size=None)
    xyz, emb, color, dirs, conf = probe_hole(stub, _frames(), opt, compound_prob_mul=False)
    assert color is None and dirs is None and xyz.shape == (6, 3) and emb.shape == (6, 32)
    raw = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0, 3.0])[:, None]
    torch.testing.assert_close(conf, raw * 0.4, rtol=1e-6, atol=0)
    assert [s[:2] for s in stub.seen] == [(1, [3, 3, 3])] * 2     # no prob_kernel_size: query_size untouched
    assert stub.opt.prob == 0 and stub.opt.query_size == [3, 3, 3]
    # an opacity threshold above every ray: nothing to grow, shapes stay [0, C]
    stub = _Stub([_frame_out(6, 4, 10.0), _frame_out(4, 1, 100.0)])
    out = probe_hole(stub, _frames(), opt, opacity_thresh=0.95)
    assert [None if t is None else tuple(t.shape) for t in out] == [(0, 3), (0, 32), (0, 3), None, (0, 1)]


def test_probe_exports_and_lego_defaults():
    import pointnerf_amd as P
    from pointnerf_amd.options import lego_opt
    assert callable(P.probe_hole) and callable(P.select_grow_candidates)
    o = lego_opt()
    assert (o.prob, o.prob_thresh, o.prob_mul, o.far_thresh) == (0, 0.7, 0.4, -1.0)
    assert (o.prob_kernel_size, o.prob_tiers, o.prob_num_step) == ([3, 3, 3], [100000], 20)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "pointnerf_amd/libpnr.so"])
    return LIB


def test_pnr_probe_validates_its_arguments_on_the_host(built):
    """Null arguments and unsupported K / SR are refused before any launch; the
    fake pointers are never dereferenced."""
    from pointnerf_amd import _lib as L
    lib = L.lib()
    assert lib.pnr_probe(*([None] * 13)) == L.PNR_EINVAL
    assert b"null" in lib.pnr_last_error()
    fake = L.c_void_p(0x1000)
    rays, qp, pts = L.Rays(), L.QueryParams(), L.Points()
    bufs = L.QueryBufs(*([fake] * 14), 0)
    rays.R, qp.SR, qp.K = 4, 80, 8
    pts.xyz = pts.emb = fake
    args = [L.ctypes.byref(rays), L.ctypes.byref(qp), L.ctypes.byref(bufs), L.ctypes.byref(pts)]
    outs = [fake] * 8   # opacity, max_opacity, max_loc_w, far_dist, avg_color, avg_dir, avg_conf, avg_emb
    assert lib.pnr_probe(*args, *outs[:7], None, None) == L.PNR_EINVAL          # avg_emb missing
    assert lib.pnr_probe(*args, *outs, None) == L.PNR_EINVAL                     # avg_color without a colour table
    assert b"absent point table" in lib.pnr_last_error()
    qp.K = 17
    assert lib.pnr_probe(*args, fake, fake, fake, fake, None, None, None, fake, None) == L.PNR_EINVAL
    assert b"K=17" in lib.pnr_last_error()
    qp.K, qp.SR = 8, 129
    assert lib.pnr_probe(*args, fake, fake, fake, fake, None, None, None, fake, None) == L.PNR_EINVAL
    assert b"SR=129" in lib.pnr_last_error()
    qp.SR, rays.R = 80, 0                                                        # no rays: no launch
    assert lib.pnr_probe(*args, fake, fake, fake, fake, None, None, None, fake, None) == L.PNR_OK
