"""render2d.hip (NeuralRenderer, fp32 and fp32h2) against float64 autograd of the
restated network (tests/nr_ref.py) on the cases no other test reaches: per-stage
fp32h2 weight scales that differ between the three stages, workgroups that take a
second, third and fourth tile in every convolution kernel, the grid-stride loops of
the absmax and rgb-gradient kernels, the weight-gradient plan at its split ceiling and
with one ragged split, one pixel, exact and ragged 128-pixel segments, fewer rows than
a tile has, all-zero features and all-zero output gradients.

The reference takes the kernel's own LeakyReLU masks (net > 0 of the forward scratch):
a pre-activation within fp32 rounding of 0 whose sign the kernel and the reference
take differently changes a gradient by a whole term, which at 143 000 pixels happens
to correct fp32 arithmetic (5e-3 of max|d x| between torch's own fp32 and fp64
restatements).  The masks are then checked on their own: a kernel's mask may differ
from z64 > 0 only where |z64| <= 8 max|z32 - z64| (the CPU fp32 restatement's noise
of that stage), and on at most 1e-4 of a stage's entries.

Every tensor -- out, d x, the ten parameter gradients -- meets the project bar (2e-5
absolute on out, 2e-5 max|ref| on a gradient) and then the tight bar 8 max(e32, 2^-22
max|ref|), e32 the CPU fp32 restatement's own error under the same masks; each line
printed is err / max(e32, 2^-22 max|ref|), so the tight bar is a ratio of 8.

Measured on one MI355X (every line of the run is in
profiles/neural_render_edges_ratios.txt), the worst ratio per path over all cases:
  fp32    2.85  (row_255, conv_layers.1.bias)
  fp32h2  2.64  (row_257, conv_rgb.1.bias)
both a bias gradient of a one-row image (a plain sum over a few hundred pixels, where
e32 is a fraction of an ulp of the sum); nothing needs more than c = 8.  Masks: at most
2 of a stage's 4.6 to 9.2 million entries differ from z64 > 0, the farthest at |z64| =
4e-7 against 8 e32 = 2e-5.

Before the stage-1 scale index was fixed in pnr_neural_render_fwd_h2 / _bwd_h2 (stage
1 read stage 2's 2^(shift - 11)), fp32h2 failed stage_1up, stage_0up, tall_5 and
tall_130_1up -- mask1, out, d x and all ten gradients, err up to max|ref| itself --
and passed every case of default-init weights; fp32 passed all.
"""
import copy
import math

import pytest
import torch

import nr_ref as NR

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp32h2")
MASK_SHARE = 1e-4            # a stage's entries whose mask may differ from z64 > 0
WORST = {}                   # precision -> (ratio, case, tensor)


def _module(name, cuda, precision):
    m, x, g = NR.case_inputs(name)
    mg = copy.deepcopy(m).to(cuda).requires_grad_(True)
    mg.precision = precision
    return mg, x.to(cuda), g.to(cuda)


def _backward(mg, x, g):
    """One autograd pass -> {out, x, the ten gradients} on the CPU."""
    mg.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    out = mg(xg)
    (out * g).sum().backward()
    got = {"out": out.detach().cpu(), "x": xg.grad.cpu()}
    got.update({n: p.grad.cpu() for n, p in mg.named_parameters()})
    return got


def _kernel_masks(mg, x):
    """The LeakyReLU masks the backward kernels will use: net0 [H, W, 64] and net1
    [H, W, 32] at the head of the forward scratch (pnr.h, fwd_scratch), > 0."""
    _, H, W, _ = x.shape
    with torch.no_grad():
        _, _, scratch = mg._fwd(x)
    f = scratch.view(torch.float32)
    net0 = f[:H * W * 64].view(1, H, W, 64)
    net1 = f[H * W * 64:H * W * 96].view(1, H, W, 32)
    return [(n > 0).permute(0, 3, 1, 2).cpu() for n in (net0, net1)]


@pytest.mark.parametrize("name,precision", [(c[0], p) for c in NR.CASES for p in PRECISIONS])
def test_edges_vs_fp64_under_the_kernels_masks(cuda, name, precision):
    mg, x, g = _module(name, cuda, precision)
    masks = _kernel_masks(mg, x)
    ref, e32 = NR.ref64_and_noise(name, masks)
    fails = []
    # the masks themselves
    for s in (0, 1):
        z64 = ref[f"z{s}"]
        diff = masks[s] != (z64 > 0)
        n = int(diff.sum())
        far = float(z64[diff].abs().max()) if n else 0.0
        print(f"{precision} {name} mask{s}: {n} of {diff.numel()} differ from z64 > 0, the farthest |z64| {far:.3e}, "
              f"8 e32 {8 * e32[f'z{s}']:.3e}")
        if far > 8 * e32[f"z{s}"]:
            fails.append(f"mask{s}: differs at |z64| = {far:.3e} > 8 e32 = {8 * e32[f'z{s}']:.3e}")
        if n > MASK_SHARE * diff.numel():
            fails.append(f"mask{s}: {n} of {diff.numel()} entries differ")
    # out, d x, the ten gradients: the project bar, then the tight bar
    got = _backward(mg, x, g)
    again = _backward(mg, x, g)
    for k in ("out",) + NR.GRADS:
        a, r = got[k], ref[k]
        assert a.shape == r.shape and a.dtype == torch.float32, k
        if not torch.isfinite(a).all():
            fails.append(f"{k}: not finite")
            continue
        scale = r.abs().max().item()
        err = (a.double() - r).abs().max().item()
        noise = max(e32[k], NR.ULP_FLOOR * scale)
        ratio = err / noise if noise > 0 else (0.0 if err == 0 else math.inf)
        print(f"{precision} {name} {k}: err {err:.3e}  e32 {e32[k]:.3e}  max|ref| {scale:.3e}  "
              f"err / max(e32, 2^-22 max|ref|) {ratio:.3f}")
        if ratio > WORST.get(precision, (-1.0,))[0]:
            WORST[precision] = (ratio, name, k)
        if err > NR.project_bar(k, scale):
            fails.append(f"{k}: err {err:.3e} > project bar {NR.project_bar(k, scale):.3e}")
        elif err > NR.tight_bar(e32[k], scale):
            fails.append(f"{k}: err {err:.3e} > tight bar {NR.tight_bar(e32[k], scale):.3e} (ratio {ratio:.2f})")
        if not torch.equal(a, again[k]):
            fails.append(f"{k}: a second run differs")
    if NR.CASE[name][5] == 0.0:      # no output gradient: every gradient is exactly 0
        for k in NR.GRADS:
            if got[k].any() or not torch.isfinite(got[k]).all():
                fails.append(f"{k}: not exactly 0 under g = 0")
    print(f"{precision} worst so far: {WORST.get(precision)}")
    assert not fails, (name, precision, fails)


def test_precisions_share_a_module(cuda):
    """One module run fp32, then fp32h2, then fp32 again (the two precisions' weight
    packs live in the same cache attributes) gives its first result bit for bit, and
    fp32h2 after fp32 what a fresh fp32h2 module gives."""
    mg, x, g = _module("stage_0up", cuda, "fp32")
    first = _backward(mg, x, g)
    mg.precision = "fp32h2"
    h2 = _backward(mg, x, g)
    mg.precision = "fp32"
    third = _backward(mg, x, g)
    fresh = _backward(_module("stage_0up", cuda, "fp32h2")[0], x, g)
    for k in first:
        assert torch.equal(first[k], third[k]), k
        assert torch.equal(h2[k], fresh[k]), k
    assert not torch.equal(first["x"], h2["x"])      # the two paths are different arithmetic
