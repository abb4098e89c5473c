"""The module's host layer without a GPU: which route a forward
takes, what it hands to the render calls under it and the dict it returns -- keys,
shapes, dtypes and sha256 of every value -- pinned by tests/golden/module_host.json,
which `python tests/test_module_host.py` recorded on the tree before the host layer
was rebuilt.

Only public seams are replaced, by recorders that return canned tensors:
render_rays, render_rays_train, render_pixels, eval_aux, probe_maps,
the 2-D renderer, the point cloud's __call__, a stub aggregator for the
seam route and ray_march.ray_march.  Nothing here depends on how renderer.py arranges
the work between them.  The canned values and the stand-ins use only exactly
rounded elementwise arithmetic, so the hashes do not depend on the CPU."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_host.json")
R, H, W = 6, 2, 3
HIT = (1, 0, 1, 1, 0, 1)      # the seam route's ray_mask; its third hit ray has no valid sample
ROUTE_OF_FIRST_CALL = dict(render_rays_train="train", render_rays="eval", render_pixels="pixels",
                           neural_points="seams")


def canned(shape, salt, dtype=torch.float32):
    """A tensor of the shape with values k / 101 that differ with salt."""
    n = int(np.prod(shape)) if len(shape) else 1
    t = ((torch.arange(n, dtype=torch.int64) * 37 + salt * 11) % 101).to(torch.float32) / 101
    return t.reshape(shape).to(dtype)


def num(v, reduce=None):
    """near / far / h / w as a recorder notes them: the Python number, however it was passed."""
    if torch.is_tensor(v):
        v = (reduce(v) if reduce else v.reshape(-1)[0]).item()
    return v


class _Cloud(SimpleNamespace):
    """The point cloud the module sees: a few attributes and the 14-tuple of a perspective query."""

    def __call__(self, inputs):
        self.log.append(["neural_points", float(num(inputs["near"], torch.min)), float(num(inputs["far"], torch.max)),
                         int(num(inputs["h"])), int(num(inputs["w"]))])
        self.types = [type(inputs[k]).__name__ for k in ("near", "far", "h", "w")]
        n_hit = sum(self.hit)
        s_loc = canned((1, n_hit, self.SR, 3), 3) * 4 + 2
        ray_mask = torch.tensor([self.hit], dtype=torch.int8)
        vsize = np.array([0.01, 0.01, 0.03125], np.float32)
        return (None,) * 8 + (s_loc, None, None, ray_mask, vsize, 0)


class _SeamAggregator(nn.Module):
    """PointAggregator for the seam route: (features, ray_valid, weight, conf_coefficient), canned."""
    C = 128

    def __init__(self, SR, K, aux):
        super().__init__()
        self.SR, self.K, self.aux = SR, K, aux
        self.w = nn.Parameter(torch.zeros(1))

    def set_rw2c(self, rw):
        pass

    def forward(self, *a):
        n = a[8].shape[1]
        feats = canned((1, n, self.SR, 129), 5)
        valid = canned((1, n, self.SR), 7) > 0.3
        if n > 2:
            valid[0, 2] = False
        weight = canned((1, n, self.SR, self.K), 9) if self.aux else None
        return feats, valid, weight, canned((1, n, self.SR, self.K), 11) if self.aux else None


def _march(ray_dist, ray_valid, feats, render_func=None, blend_func=None, bg_color=None):
    """ray_march's 7-tuple from exactly rounded elementwise arithmetic (a stand-in, not a march)."""
    op = torch.clamp(feats[..., 0] * ray_dist * 8, 0, 1) * ray_valid
    bg_t = 1 - op[..., :1]
    color = op[..., :1] * feats[..., 0, 1:] + (0 if bg_color is None else bg_t * bg_color.reshape(-1))
    return color, feats[..., 1:], op, 1 - op, (op * 0.5)[..., None], bg_t, bg_t


class _Render2d(nn.Module):
    def forward(self, x):
        return x[..., :3] * 0.5


def _inputs(**over):
    inp = dict(campos=canned((1, 3), 1), raydir=canned((1, R, 3), 2), bg_color=canned((128,), 4),
               camrotc2w=torch.eye(3)[None], near=torch.tensor([[2.0, 2.5]]), far=torch.tensor([[5.5, 6.0]]))
    inp.update(over)
    return inp


def _pinputs(**over):
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pix = torch.from_numpy(np.stack([xs, ys], -1).reshape(1, -1, 2)).long()
    k = torch.tensor([[[50.0, 0, 1.5], [0, 50.0, 1.0], [0, 0, 1]]])
    return _inputs(**dict(dict(pixel_idx=pix, h=torch.tensor([H]), w=torch.tensor([W]), intrinsic=k), **over))


def _cases():
    """name -> (opt overrides, module settings, inputs).  Module settings: perspective, fused, train,
    grad, hit, rays (world: the recorders' batch size)."""
    no_aux, aux = dict(zero_one_loss_items=[], sparse_loss_weight=0), dict(zero_one_loss_items=["conf_coefficient"])
    p = dict(wcoord_query=0, SR=24, K=8, shpnt_jitter="passfunc")
    c = {}
    for tag, o in (("", no_aux), (" aux", aux)):
        c["world eval" + tag] = (o, {}, _inputs())
        c["world train" + tag] = (o, dict(train=True), _inputs())
        c["seams hit" + tag] = ({**p, **o}, dict(perspective=True), _pinputs())
    c["world eval sparse aux"] = (dict(zero_one_loss_items=[], sparse_loss_weight=0.1), {}, _inputs())
    c["world eval float near far"] = (no_aux, {}, _inputs(near=2.0, far=6.0))
    c["world eval train() under no_grad"] = (no_aux, dict(train=True, grad=False), _inputs())
    c["world eval probe"] = ({**no_aux, "prob": 1}, {}, _inputs())
    c["world eval probe R=0"] = ({**no_aux, "prob": 1}, dict(rays=0), _inputs(raydir=torch.zeros((1, 0, 3))))
    c["world eval bg_ray"] = (no_aux, {}, _inputs(bg_ray=canned((1, R, 3), 6)))
    c["world eval cnn tensor hw"] = ({**no_aux, "neural_render": "cnn"}, {},
                                     _inputs(h=torch.tensor([H]), w=torch.tensor([W])))
    c["world eval cnn int hw"] = ({**no_aux, "neural_render": "cnn"}, {}, _inputs(h=H, w=W))
    c["seams no hit"] = ({**p, **aux}, dict(perspective=True, hit=(0,) * R), _pinputs())
    c["seams bg_ray"] = ({**p, **no_aux}, dict(perspective=True), _pinputs(bg_ray=canned((1, R, 3), 6)))
    c["seams cnn"] = ({**p, **no_aux, "neural_render": "cnn"}, dict(perspective=True), _pinputs())
    c["pixels taken"] = ({**p, **no_aux}, dict(perspective=True, fused=True), _pinputs())
    c["pixels taken float near far int hw"] = ({**p, **no_aux}, dict(perspective=True, fused=True),
                                               _pinputs(near=2.0, far=6.0, h=H, w=W))
    c["pixels taken is_train passfunc"] = ({**p, **no_aux, "is_train": 1}, dict(perspective=True, fused=True),
                                           _pinputs())
    c["pixels taken cnn"] = ({**p, **no_aux, "neural_render": "cnn"}, dict(perspective=True, fused=True), _pinputs())
    c["pixels declined: training step"] = ({**p, **no_aux}, dict(perspective=True, fused=True, train=True), _pinputs())
    c["pixels declined: aux wanted"] = ({**p, **aux}, dict(perspective=True, fused=True), _pinputs())
    c["pixels declined: jitter"] = ({**p, **no_aux, "is_train": 1, "shpnt_jitter": "uniform"},
                                    dict(perspective=True, fused=True), _pinputs())
    # the refusals
    c["refused: pixels declined: prob == 1"] = ({**p, **no_aux, "prob": 1}, dict(perspective=True, fused=True),
                                                _pinputs())
    c["refused: B > 1"] = (no_aux, {}, _inputs(raydir=canned((2, R, 3), 2)))
    c["refused: probe while training"] = ({**no_aux, "prob": 1}, dict(train=True), _inputs())
    c["refused: probe on perspective"] = ({**p, **no_aux, "prob": 1}, dict(perspective=True), _pinputs())
    for name in ("pixel_idx", "h", "w", "intrinsic"):
        c["refused: pixels without " + name] = ({**p, **no_aux}, dict(perspective=True, fused=True),
                                                _pinputs(**{name: None}))
    return c


def _build(opt_over, perspective=False, fused=False, train=False, grad=None, hit=HIT, rays=R):
    """(module, log): the module of a case with its recorders in place."""
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.renderer import NeuralPointsRayMarching
    opt = lego_opt(**opt_over)
    SR, K = int(opt.SR), int(opt.K)
    log = []
    cloud = _Cloud(device=torch.device("cpu"), perspective=perspective, Rw2c=torch.eye(3), xyz=torch.zeros((5, 3)),
                   points_conf=None, log=log, hit=hit, SR=SR, types=None)
    agg = _SeamAggregator(SR, K, None) if perspective else PointAggregator(opt)
    m = NeuralPointsRayMarching(opt, cloud, agg, **(dict(fused_perspective=True) if fused else {}))
    if perspective:
        agg.aux = m.wants_aux()
    m.train(train)
    if m.neural_render_2d is not None:
        m.neural_render_2d = _Render2d()
    four = (canned((rays, 128), 21), canned((rays, SR), 22), canned((rays,), 23),
            (canned((rays,), 24) > 0.5).to(torch.int8))
    aux3 = dict(weight=canned((1, 4, SR, K), 25), blend_weight=canned((1, 4, SR, 1), 26),
                conf_coefficient=canned((1, 4, SR, K), 27))

    def scal(near, far):
        return [float(num(near, torch.min)), float(num(far, torch.max))]

    def render_rays(campos, camrot, raydir, near, far, bg_color, **kw):
        log.append(["render_rays", list(raydir.shape)] + scal(near, far) + [bg_color is not None])
        return four

    def render_rays_train(campos, camrot, raydir, near, far, bg_color):
        log.append(["render_rays_train", list(raydir.shape)] + scal(near, far) + [bg_color is not None])
        m.last_train_aux = dict(aux3, sample_pidx=None)
        return four

    def eval_aux(campos, camrot, raydir, near, far, opacity):
        log.append(["eval_aux", list(raydir.shape)] + scal(near, far) + [opacity is four[1]])
        return dict(aux3, sample_pidx=None)

    def probe_maps(campos, camrot, raydir, near, far, opacity):
        from pointnerf_amd.renderer import PROBE_KEYS
        log.append(["probe_maps", list(raydir.shape)] + scal(near, far) + [opacity is four[1]])
        c = dict(zip(PROBE_KEYS, (1, 3, 1, 3, 3, 1, 32)))
        return {k: None if k == "shading_avg_dir" else canned((1, rays, c[k]), 30 + i)
                for i, k in enumerate(PROBE_KEYS)}

    valid = canned((rays,), 28) > 0.4

    def note_pixels(pix, h, w, intr, near, far, bg_color):
        log.append(["render_pixels", None if pix is None else list(pix.reshape(-1, 2).shape), int(num(h)), int(num(w)),
                    np.asarray(intr.detach().cpu() if torch.is_tensor(intr) else intr,
                               np.float32).reshape(-1, 3, 3)[0].tolist()] + scal(near, far) + [bg_color is not None])

    def render_pixels(campos, camrot, pix, h, w, intr, near, far, bg_color, frame=False, **kw):
        note_pixels(pix, h, w, intr, near, far, bg_color)
        m.pixel_types = [type(v).__name__ for v in (near, far, h, w)]
        if frame:
            from pointnerf_amd.renderer import Frame
            return Frame(*four, ray_valid=valid)
        m._pixel_ray_valid = valid   # the recording branch: the tree before the rebuild hands ray_valid over here
        return four

    m.render_pixels = render_pixels
    m.render_rays, m.render_rays_train, m.eval_aux, m.probe_maps = render_rays, render_rays_train, eval_aux, probe_maps
    m.grad = (train if grad is None else grad)
    return m, log


def _enc(v):
    if torch.is_tensor(v):
        a = np.ascontiguousarray(v.detach().numpy())
        return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
    return v


def _observe(case, monkeypatch_march):
    from pointnerf_amd._lib import PnrError
    opt_over, setup, inp = case
    m, log = _build(opt_over, **setup)
    monkeypatch_march()
    res = {"error": None, "out": None}
    try:
        with torch.set_grad_enabled(m.grad):
            out = m(**inp)
        res["out"] = [[k, _enc(v)] for k, v in out.items()]      # a list: the keys' order is part of it
    except PnrError as e:
        res["error"] = str(e)
    except RuntimeError:          # torch's own: its wording is not the project's
        res["error"] = "RuntimeError"
    res["calls"] = log
    res["route"] = ROUTE_OF_FIRST_CALL[log[0][0]] if log else None
    return res, m


def _patch_march():
    import pointnerf_amd.ray_march  # noqa: F401  (the package exports the function under the same name)
    RM = sys.modules["pointnerf_amd.ray_march"]
    RM.ray_march = _march


@pytest.fixture
def march(monkeypatch):
    import pointnerf_amd.ray_march  # noqa: F401  (the package exports the function under the same name)
    RM = sys.modules["pointnerf_amd.ray_march"]
    return lambda: monkeypatch.setattr(RM, "ray_march", _march)


@pytest.mark.parametrize("name", sorted(_cases()))
def test_forward_does_what_the_fixture_recorded(march, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got, m = _observe(_cases()[name], march)
    got = json.loads(json.dumps(got))
    for k in ("error", "route", "calls", "out"):
        assert got[k] == want[k], (name, k)


def test_fixture_shows_the_routes_and_the_dicts():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(_cases())
    routes = None
    routes = {k: v["route"] for k, v in want.items()}
    assert routes["world eval"] == "eval" and routes["world train aux"] == "train"
    assert routes["world eval train() under no_grad"] == "eval"
    assert routes["seams hit"] == routes["seams no hit"] == "seams"
    assert [routes[k] for k in sorted(routes) if k.startswith("pixels taken")] == ["pixels"] * 4
    assert [routes[k] for k in sorted(routes) if k.startswith("pixels declined")] == ["seams"] * 3
    # an empty world batch never worked: view(1, 0, -1) is ambiguous to torch (DESIGN.md 30 keeps it so)
    assert want.pop("world eval probe R=0") == dict(error="RuntimeError", out=None, route="eval", calls=[
        ["render_rays", [0, 3], 2.0, 6.0, True], ["eval_aux", [0, 3], 2.0, 6.0, True]])
    for k, v in want.items():
        assert (v["error"] is not None) == k.startswith("refused") == (v["out"] is None), k
        assert not k.startswith("refused") or v["calls"] == [], k
    base = ["coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "ray_mask", "coarse_mask",
            "queried_shading"]
    aux = ["weight", "blend_weight", "conf_coefficient"]
    keys = {k: [kv[0] for kv in v["out"]] for k, v in want.items() if v["out"]}
    assert keys["world eval"] == keys["seams hit"] == keys["pixels taken"] == base
    assert keys["world eval aux"] == keys["world train aux"] == keys["seams hit aux"] == base + aux
    assert keys["world eval probe"][:6] == base and len(keys["world eval probe"]) == 6 + 3 + 7
    assert keys["world eval cnn int hw"] == keys["seams cnn"] == keys["pixels taken cnn"] == \
        base + ["final_coarse_raycolor"]
    assert want["world eval cnn int hw"]["out"] == want["world eval cnn tensor hw"]["out"]
    calls = {k: [c[0] for c in v["calls"]] for k, v in want.items()}
    assert calls["world eval aux"] == ["render_rays", "eval_aux"]
    assert calls["world eval probe"] == ["render_rays", "eval_aux", "probe_maps"]
    assert calls["world eval bg_ray"][0] == "render_rays" and want["world eval bg_ray"]["calls"][0][-1] is False
    # near = min, far = max of the tensors; the seams' no-hit batch still fills every row
    assert want["world eval"]["calls"][0][2:4] == [2.0, 6.0] == want["seams hit"]["calls"][0][1:3]
    shapes = {kv[0]: kv[1]["shape"] for kv in want["seams no hit"]["out"]}
    assert shapes["coarse_raycolor"] == [1, R, 128] and shapes["weight"][:2] == [1, 0]


def test_route_and_assembly_exist_once(march, monkeypatch):
    """Every route's dict is made by the one assemble, after the one route."""
    from pointnerf_amd.renderer import NeuralPointsRayMarching as M
    seen = []
    route, assemble = M.route, M.assemble

    def noted_route(self, inputs):
        r = route(self, inputs)
        seen.append(("route", r[0]))
        return r

    def noted_assemble(self, frame, inputs=None):
        seen.append(("assemble", type(frame).__name__))
        return assemble(self, frame, inputs)

    monkeypatch.setattr(M, "route", noted_route)
    monkeypatch.setattr(M, "assemble", noted_assemble)
    for name, case in sorted(_cases().items()):
        del seen[:]
        got, m = _observe(case, march)
        if got["error"] is None:
            assert seen == [("route", got["route"]), ("assemble", "Frame")], name
            assert m.path == got["route"] and isinstance(m.path_why, str), name
    for fn in ("_forward_perspective", "_forward_pixels", "_fused_forward_applies"):
        assert not hasattr(M, fn)


def test_numbers_are_read_once_at_the_top(march):
    """Intended change: below forward, near / far / h / w are Python numbers (the perspective routes read the
    tensors a second time before)."""
    cases = _cases()
    _, m = _observe(cases["seams hit"], march)
    assert m.neural_points.types == ["float", "float", "int", "int"]
    _, m = _observe(cases["pixels taken"], march)
    assert m.pixel_types == ["float", "float", "int", "int"]


def test_module_is_freed_without_the_cyclic_collector():
    """The module owns the query buffers, the scratch and, through the cloud, the grid: dropping the last
    reference frees it at once (nothing it holds refers back to it)."""
    import gc
    import weakref
    from pointnerf_amd.aggregator import PointAggregator
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.renderer import NeuralPointsRayMarching
    opt = lego_opt()
    cloud = SimpleNamespace(device=torch.device("cpu"), perspective=False, Rw2c=torch.eye(3), xyz=torch.zeros((5, 3)))
    was_on = gc.isenabled()
    gc.disable()
    try:
        m = NeuralPointsRayMarching(opt, cloud, PointAggregator(opt))
        assert m.finish() == [] and m._pending == [] and m._sv_per_ray is None
        alive = weakref.ref(m)
        del m
        assert alive() is None
    finally:
        if was_on:
            gc.enable()


def test_conf_losses_refuse_before_a_training_render():
    """Intended change: zero_one_conf_loss refuses as sparse_conf_loss does (it dereferenced None)."""
    from pointnerf_amd._lib import PnrError
    m, _ = _build(dict(zero_one_loss_items=["conf_coefficient"]))
    for fn in (m.zero_one_conf_loss, m.sparse_conf_loss):
        with pytest.raises(PnrError, match=fn.__name__ + ": no training render yet"):
            fn()


def test_neural_points_is_reexported():
    import pointnerf_amd
    from pointnerf_amd import neural_points, renderer
    assert renderer.NeuralPoints is neural_points.NeuralPoints is pointnerf_amd.NeuralPoints


def test_perspective_refusals_are_stated_once():
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.querier_p import check_supported, frustum_geometry
    p = dict(wcoord_query=0, vscale=[2, 2, 1], kernel_size=[3, 3, 3], query_size=[3, 3, 3])
    k = np.array([[50.0, 0, 1.5], [0, 50.0, 1.0], [0, 0, 1]], np.float32)
    for over, msg in ((dict(inverse=1), "--inverse 1"), (dict(NN=0), "NN == 0"),
                      (dict(kernel_size=[5, 5, 3]), "wider than query_size"),
                      (dict(shpnt_jitter="sideways"), "shpnt_jitter")):
        for entry in (check_supported, lambda o: frustum_geometry(o, H, W, k, 2.0, 6.0)):
            with pytest.raises(PnrError, match=msg):
                entry(lego_opt(**{**p, **over}))
    assert check_supported(lego_opt(**p)) == "passfunc"


if __name__ == "__main__":   # record the fixture (run on the tree whose behaviour is to be kept)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests", "golden")]
    obs = {name: _observe(case, _patch_march)[0] for name, case in sorted(_cases().items())}
    with open(GOLDEN, "w") as f:
        json.dump(obs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: " + ", ".join(f"{k} -> {v['route'] or 'refused'}" for k, v in obs.items()))
