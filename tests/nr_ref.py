"""Torch-convolution restatement of the fork's 2-D neural renderer
(models/neural_render/neural_renderer.py:81-104): the checker of
pointnerf_amd.neural_render.NeuralRenderer in the tests (test infrastructure,
not product code; parity unpinned: the reference module needs kornia).

``neural_render_torch`` is the plain restatement.  The rest is the float64
reference of tests/test_gpu_neural_render_edges.py: ``render_ref`` restates the
same network with the LeakyReLU masks handed in (a kernel and a reference that
disagree on the sign of a pre-activation within rounding of 0 differ by a
whole term, not by rounding, so the reference takes the kernel's own masks and
the masks are checked on their own), ``CASES`` names the image sizes and
per-stage weight factors, ``ref64_and_noise`` gives the float64 autograd of
sum(out * g) with the error of the same restatement in float32 on the CPU (the
yardstick of ``tight_bar``), and ``emulate`` restates forward and backward
stage by stage in float32 with one kernel bug at a time (tests/test_nr_ref_host.py).
"""
import copy
import hashlib
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F


def neural_render_torch(mod, x):
    """rgb [1, H, W, 3] of ``mod``'s parameters on x [1, H, W, 128] with torch
    convolutions (autograd path, any dtype / device)."""
    x = x.permute(0, 3, 1, 2)
    rgb = mod.conv_rgb[0](x)
    net = x
    for i, layer in enumerate(mod.conv_layers):
        net = F.leaky_relu(layer(net), 0.2)
        rgb = rgb + mod.conv_rgb[i + 1](net)
    return torch.sigmoid(rgb).permute(0, 2, 3, 1)


def render_ref(mod, x, masks=None):
    """(rgb [1, H, W, 3], [z0, z1]) of ``mod`` on x [1, H, W, 128] in the module's
    dtype: neural_render_torch with the pre-activations z0 [1, 64, H, W] and z1
    [1, 32, H, W] returned.  masks = [m0, m1] (bool, the shapes of z0 / z1): the
    activation is where(m, z, 0.2 z); None: leaky_relu (then bitwise
    neural_render_torch)."""
    x = x.permute(0, 3, 1, 2)
    rgb = mod.conv_rgb[0](x)
    net = x
    zs = []
    for i, layer in enumerate(mod.conv_layers):
        z = layer(net)
        zs.append(z)
        net = F.leaky_relu(z, 0.2) if masks is None else torch.where(masks[i], z, 0.2 * z)
        rgb = rgb + mod.conv_rgb[i + 1](net)
    return torch.sigmoid(rgb).permute(0, 2, 3, 1), zs


# ------------------------------------------------------------------- the cases
BAR = 2e-5                   # the project bar: 2e-5 absolute on out, 2e-5 * max|ref| on a gradient
ULP_FLOOR = 2.0 ** -22       # a few fp32 ulps of a tensor's largest entry
C_TIGHT = 8.0                # aggregate_ref.C_TIGHT: the margin a split GEMM gets over an fp32 one
X_SCALE = 0.5                # tests/test_gpu_neural_render.py's feature magnitude
ONE = (1.0, 1.0, 1.0)
UP1 = (1.0, 4.0, 0.25)       # h2 shifts -9 / -6 / -10
UP0 = (8.0, 0.5, 2.0)        # h2 shifts -6 / -9 / -7

# (name, H, W, (f0, f1, f2), x_scale, g_scale).  f_s multiplies both convs of stage s
# (weights and biases; trunk and rgb for stages 0 and 1, conv_rgb.2 for stage 2).
# x_scale: a number, or (s_top, rows, s_rest): the first ``rows`` image rows times
# s_top, the others times s_rest.
CASES = (
    ("stage_1up", 64, 64, UP1, X_SCALE, 1.0),
    ("stage_0up", 40, 150, UP0, X_SCALE, 1.0),
    ("tall_5", 3000, 5, UP1, X_SCALE, 1.0),
    # rows 0..950 four times the rest: they reach no further than row 951, the end of the
    # h2 tiles 0..475 whose workgroups go on to a second tile, so the maximum of net0 is
    # well above that of every workgroup's last tile
    ("tall_5_top4", 3000, 5, ONE, (4 * X_SCALE, 951, X_SCALE), 1.0),
    ("tall_130", 1100, 130, ONE, X_SCALE, 1.0),
    ("tall_130_1up", 1100, 130, UP1, X_SCALE, 1.0),
    # three segments and 1035 one-row tiles: a workgroup of the 1024 of the d x
    # convolution goes from segment 0 to segment 1 (1024 % 3 = 1)
    ("segs_3", 345, 257, ONE, X_SCALE, 1.0),
    ("px_1", 1, 1, ONE, X_SCALE, 1.0),
    ("row_128", 1, 128, ONE, X_SCALE, 1.0),
    ("two_129", 2, 129, ONE, X_SCALE, 1.0),
    ("three_257", 3, 257, ONE, X_SCALE, 1.0),
    ("five_127", 5, 127, ONE, X_SCALE, 1.0),
    ("row_255", 1, 255, ONE, X_SCALE, 1.0),
    ("row_256", 1, 256, ONE, X_SCALE, 1.0),
    ("row_257", 1, 257, ONE, X_SCALE, 1.0),
    ("x_zero", 7, 129, ONE, 0.0, 1.0),
    ("x_zero_b0", 7, 129, ONE, 0.0, 1.0),
    ("g_zero", 7, 129, ONE, X_SCALE, 0.0),
)
CASE = {c[0]: c for c in CASES}
ZERO_TRUNK_BIAS = ("x_zero_b0",)     # conv_layers.{0,1}.bias = 0: every pre-activation is exactly 0
PARAMS = ("conv_layers.0.weight", "conv_layers.0.bias", "conv_layers.1.weight", "conv_layers.1.bias",
          "conv_rgb.0.weight", "conv_rgb.0.bias", "conv_rgb.1.weight", "conv_rgb.1.bias",
          "conv_rgb.2.weight", "conv_rgb.2.bias")
GRADS = ("x",) + PARAMS
ENTRIES = ("out",) + GRADS + ("z0", "z1")

# render2d.hip's tile loops and plans, restated for the cases' own checks
SEG = 128                    # pixels of a row per tile (kRPx, kHPx)
GRID_F32, GRID_H2 = 768, 1024
RO_H2, RO_H2_DX = 2, 1       # output rows per h2 tile; the 4-row-tile d x convolution
ABSMAX_GRID_PX = 8192        # k_nr_absmax: 1024 workgroups x 256 threads x 4 floats / 128 channels
RGB_GRAD_H2_GRID_PX = 131072   # k_nr_rgb_grad_h2: 512 workgroups x 256 threads


def cdiv(a, b):
    return -(-a // b)


def tiles(H, W, ro):
    return cdiv(H, ro) * cdiv(W, SEG)


def wgrad_plan(npix, px=32):
    """render2d.hip's wgrad_plan: (splits, pixels per split)."""
    s = min(cdiv(512, 3), cdiv(max(npix, 1), 8 * px))
    ch = cdiv(cdiv(max(npix, 1), s), px) * px
    return (cdiv(npix, ch) if npix > 0 else 1), ch


_INPUTS = {}


def case_inputs(name):
    """(module, x [1, H, W, 128], g [1, H, W, 3]) of a case: fp32 on the CPU, seeded,
    the same on every call (callers copy before they change anything)."""
    if name not in _INPUTS:
        from pointnerf_amd.neural_render import NeuralRenderer
        _, H, W, fs, xs, gs = CASE[name]
        gen = torch.Generator().manual_seed(1000 + [c[0] for c in CASES].index(name))
        state = torch.random.get_rng_state()
        torch.manual_seed(int(torch.randint(1 << 30, (1,), generator=gen)))
        m = NeuralRenderer(input_dim=128)
        torch.random.set_rng_state(state)
        with torch.no_grad():
            for s, f in enumerate(fs):
                for cv in ([m.conv_layers[s]] if s < 2 else []) + [m.conv_rgb[s]]:
                    cv.weight *= f
                    cv.bias *= f
            if name in ZERO_TRUNK_BIAS:
                for cv in m.conv_layers:
                    cv.bias.zero_()
        x = torch.randn((1, H, W, 128), generator=gen)
        if isinstance(xs, tuple):
            x[:, :xs[1]] *= xs[0]
            x[:, xs[1]:] *= xs[2]
        else:
            x *= xs
        g = torch.randn((1, H, W, 3), generator=gen) * gs
        m.requires_grad_(False)
        _INPUTS[name] = (m, x, g)
    return _INPUTS[name]


def shifts(name):
    """(forward, transposed) fp32h2 shifts of the case's three stacked stages, as
    NeuralRenderer.packed_h2 / packed_t_h2 pick them (aggregator.h2_shift of the
    stacked weights)."""
    from pointnerf_amd.aggregator import h2_shift
    m = case_inputs(name)[0]
    fwd = [h2_shift(m._stack(*st)[0].permute(0, 2, 3, 1).reshape(st[2], -1)) for st in m._stages()]
    bwd = [h2_shift(m._stack_t(*st)) for st in m._stages()]
    return fwd, bwd


def _run(name, masks, dtype):
    m, x, g = case_inputs(name)
    md = copy.deepcopy(m).to(dtype).requires_grad_(True)
    xr = x.to(dtype, copy=True).requires_grad_(True)
    out, zs = render_ref(md, xr, masks)
    (out * g.to(dtype)).sum().backward()
    r = {"out": out.detach(), "x": xr.grad, "z0": zs[0].detach(), "z1": zs[1].detach()}
    r.update({n: p.grad for n, p in md.named_parameters()})
    return {k: r[k].double() for k in ENTRIES}


_FWD64 = OrderedDict()


def forward64(name):
    """[z0, z1] of the case's float64 forward with leaky_relu (no masks handed in)."""
    if name not in _FWD64:
        m, x, _ = case_inputs(name)
        with torch.no_grad():
            _FWD64[name] = render_ref(copy.deepcopy(m).double(), x.double())[1]
        while len(_FWD64) > 2:
            _FWD64.popitem(last=False)
    return _FWD64[name]


def masks64(name):
    return [z > 0 for z in forward64(name)]


_REF = OrderedDict()


def ref64_and_noise(name, masks):
    """(ref, e32) of a case under the given LeakyReLU masks: ref = float64 autograd of
    sum(out * g) -- out [1, H, W, 3], x (d x) [1, H, W, 128], the ten parameter
    gradients, the pre-activations z0 / z1 -- and e32[k] = max|ref32[k] - ref[k]| of
    the same restatement in float32 on the CPU.  Cached on the masks' bits (the two
    precisions of a case share it when their masks agree); callers leave it unchanged."""
    h = hashlib.blake2b(digest_size=16)
    for mk in masks:
        h.update(np.packbits(mk.cpu().numpy()).tobytes())
    key = (name, h.hexdigest())
    if key not in _REF:
        masks = [mk.cpu() for mk in masks]
        ref = _run(name, masks, torch.float64)
        r32 = _run(name, masks, torch.float32)
        _REF[key] = (ref, {k: (r32[k] - ref[k]).abs().max().item() for k in ENTRIES})
        while len(_REF) > 2:
            _REF.popitem(last=False)
    return _REF[key]


def tight_bar(e32, scale, c=C_TIGHT):
    return c * max(e32, ULP_FLOOR * scale)


def project_bar(k, scale):
    return BAR if k == "out" else BAR * scale


# ------------------------------------------------- float32 emulation with one bug
MUTATIONS = ("scale_fwd", "scale_bwd", "acc_not_cleared", "stale_x0", "halo_col128", "drop_odd_row",
             "drop_last_split", "bias_octet", "mask_ge", "amax_last_tile")


def _img_scale(m):
    """render2d.hip's img_scale: 2^e with m 2^e in [2^14, 2^15)."""
    return 1.0 if not (m > 0) else 2.0 ** (15 - math.frexp(m)[1])


def emulate(name, masks, mut=None, dtype=torch.float32):
    """The entries of ref64_and_noise (out, d x, the ten gradients, z0, z1) computed
    stage by stage as render2d.hip does -- per stage one convolution of the stacked
    [trunk; rgb] rows, data gradients as transposed convolutions of the stacked
    [dz; g] image, weight gradients as sums over the pixels -- in ``dtype`` on the
    CPU, with the bug ``mut`` (None: none):
      scale_fwd        stage 1's forward products times 2^(s2 - s1) (stage 2's scale)
      scale_bwd        stage 1's data gradient times 2^(s2 - s1) of the transposed packs
      acc_not_cleared  stage 0 forward, 2-row tiles, 1024 workgroups: the tile at
                       t + 1024 adds the products of the tile at t
      stale_x0         the d x convolution, 1-row tiles, 1024 workgroups: the tile at
                       t + 1024 staged at the segment of the tile at t
      halo_col128      stage 0 forward: output column 128 reads column 127 as 0
      drop_odd_row     stage 0 forward: the last row of an odd H is not written (0)
      drop_last_split  stage 0 weight and bias gradients: the ragged last split dropped
      bias_octet       stage 0 bias gradients: pixels 24..31 missing
      mask_ge          the backward's masks taken as z >= 0
      amax_last_tile   stage 1 staged in f16 with the scale of the maximum over the
                       workgroups' last tiles (2-row tiles, 1024 workgroups)"""
    assert mut is None or mut in MUTATIONS
    m, x, g = case_inputs(name)
    _, H, W, _, _, _ = CASE[name]
    P = {n: p.detach().to(dtype) for n, p in m.named_parameters()}
    xi = x.to(dtype).permute(0, 3, 1, 2)
    gi = g.to(dtype).permute(0, 3, 1, 2)
    segs = cdiv(W, SEG)
    fs, bs = shifts(name) if mut in ("scale_fwd", "scale_bwd") else (None, None)

    def stacked(s, what):
        names = ([f"conv_layers.{s}.{what}"] if s < 2 else []) + [f"conv_rgb.{s}.{what}"]
        return torch.cat([P[n] for n in names], 0)

    def act(z, mk):
        return torch.where(mk, z, 0.2 * z)

    # ---- forward
    zs, nets, rgb, inp = [], [xi], None, xi
    for s in range(3):
        cout = (64, 32, 0)[s]
        Ws = stacked(s, "weight")
        if mut == "amax_last_tile" and s == 1:
            nt = tiles(H, W, RO_H2)
            first_last = max(nt - GRID_H2, 0)          # tiles from here on are some workgroup's last
            assert segs == 1
            mx = inp[:, :, first_last * RO_H2:].abs().max().item()
            xs = _img_scale(mx)
            inp = torch.where((inp * xs).abs() >= 65520.0, torch.sign(inp) * math.inf, inp)   # f16 overflow
        y = F.conv2d(inp, Ws, None, 1, 1)
        if mut == "scale_fwd" and s == 1:
            y = y * 2.0 ** (fs[2] - fs[1])
        if mut == "acc_not_cleared" and s == 0:
            assert segs == 1 and tiles(H, W, RO_H2) > GRID_H2
            r0 = GRID_H2 * RO_H2
            y = torch.cat([y[:, :, :r0], y[:, :, r0:] + y[:, :, :H - r0]], 2)
        if mut == "halo_col128" and s == 0:
            assert W > SEG
            cut = inp.clone()
            cut[..., SEG - 1] = 0
            y = y.clone()
            y[..., SEG] = F.conv2d(cut, Ws, None, 1, 1)[..., SEG]
        y = y + stacked(s, "bias").view(1, -1, 1, 1)
        if mut == "drop_odd_row" and s == 0:
            assert H % 2 == 1
            y = y.clone()
            y[:, :, H - 1] = 0
        rgb = y[:, cout:] if rgb is None else rgb + y[:, cout:]
        if s < 2:
            zs.append(y[:, :cout])
            inp = act(zs[s], masks[s])
            nets.append(inp)
    out = torch.sigmoid(rgb)
    if mut == "mask_ge":
        masks = [z >= 0 for z in zs]
    # ---- backward
    gr = gi * out * (1 - out)
    res = {"out": out.permute(0, 2, 3, 1), "z0": zs[0], "z1": zs[1]}
    dz = None
    for s in (2, 1, 0):
        cout = (64, 32, 0)[s]
        Ws = stacked(s, "weight")
        dY = gr if s == 2 else torch.cat([dz, gr], 1)
        dYw = dY
        npix = H * W
        if mut == "drop_last_split" and s == 0:
            ns, ch = wgrad_plan(npix, 32)
            assert ns >= 2 and npix % ch
            dYw = dY.clone()
            dYw.view(1, -1, npix)[:, :, (ns - 1) * ch:] = 0
        dW = torch.nn.grad.conv2d_weight(nets[s], Ws.shape, dYw, padding=1)
        db = dYw.sum((0, 2, 3))
        if mut == "bias_octet" and s == 0:
            assert npix >= 32
            db = db - dY.reshape(1, -1, npix)[0, :, 24:32].sum(1)
        if s < 2:
            res[f"conv_layers.{s}.weight"], res[f"conv_layers.{s}.bias"] = dW[:cout], db[:cout]
        res[f"conv_rgb.{s}.weight"], res[f"conv_rgb.{s}.bias"] = dW[cout:], db[cout:]
        dn = F.conv_transpose2d(dY, Ws, None, 1, 1)
        if mut == "scale_bwd" and s == 1:
            dn = dn * 2.0 ** (bs[2] - bs[1])
        if mut == "stale_x0" and s == 0:
            nt = tiles(H, W, RO_H2_DX)
            assert nt > GRID_H2 and GRID_H2 % segs
            wide = F.conv_transpose2d(F.pad(dY, (0, segs * SEG + 1 - W)), Ws, None, 1, 1)
            dn = dn.clone()
            for t in range(GRID_H2, nt):
                y, sg, sp = t // segs, t % segs, (t - GRID_H2) % segs
                n = min(SEG, W - sg * SEG)
                dn[:, :, y, sg * SEG:sg * SEG + n] = wide[:, :, y, sp * SEG:sp * SEG + n]
        if s > 0:
            dz = dn * torch.where(masks[s - 1], 1.0, 0.2).to(dtype)
        else:
            res["x"] = dn.permute(0, 2, 3, 1)
    return {k: res[k].double() for k in ENTRIES}


def worst_over_tight(got, ref, e32):
    """(ratio, entry): the worst max|got - ref| / tight bar over the entries (inf where
    ``got`` is not finite)."""
    worst = (0.0, None)
    for k in ENTRIES:
        scale = ref[k].abs().max().item()
        err = (got[k] - ref[k]).abs().max().item()
        if not math.isfinite(err):
            return math.inf, k
        bar = tight_bar(e32[k], scale)
        r = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
        worst = max(worst, (r, k), key=lambda t: t[0])
    return worst
