"""pointnerf_amd.optim.Adam (pnr_adam_step) vs torch.optim.Adam, the
optimizer of the reference's finetune loop (train_ddp.py;
mvs_points_volumetric_model.py:102-123).  Same update order as torch's
fused kernel (m, v by fma, denom = sqrt(v) / sqrt(bc2) + eps, addcdiv); the
two differ only by fp32 rounding of the contracted terms, so the bar is
|d| <= 1e-6 |ref| + 1e-9 for the parameters after several steps (their own
ulp is ~1e-7 relative) and 1e-6 of |ref| + 1e-6 of the tensor's largest entry
for the moments (a moment near 0 is the cancellation of larger terms).

test_adam_many_tensors_across_launches passes one group of 70 tensors (three
launches of up to 32, each with its own chunk table; numels on both sides of the
float4 quad, the 1024-element pass and the 8192-element chunk, an empty tensor,
aligned and unaligned tensors in one launch): bitwise equal to single-tensor
launches on an MI355X, and inside the same bars against torch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(100003,), (2000, 39), (1,), (37, 3), (256, 284), (4096,)]
    return [torch.randn(s, generator=g).to(dev) for s in shapes]


def _grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g).to(p.device) * 10 ** float(torch.randint(-6, 2, (1,), generator=g))
            for p in ps]


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("fused", [True, False])
def test_adam_matches_torch(cuda, wd, fused):
    from pointnerf_amd.optim import Adam
    a = [torch.nn.Parameter(p) for p in _params(cuda, 0)]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    mine = Adam(a, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref = torch.optim.Adam(b, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, fused=fused,
                           foreach=None if fused else False)
    v0 = [p._version for p in a]
    for it in range(6):
        gs = _grads(a, 100 + it)
        for p, q, g in zip(a, b, gs):
            p.grad, q.grad = g.clone(), g.clone()
        if it == 3:   # a parameter without a gradient this step: untouched, its step count lags
            a[2].grad = b[2].grad = None
        mine.step()
        ref.step()
    assert all(p._version > v for p, v in zip(a, v0))   # caches keyed on the version see the update
    for i, (p, q) in enumerate(zip(a, b)):
        d = (p.detach() - q.detach()).abs()
        tol = 1e-6 * q.detach().abs() + 1e-9
        assert bool((d <= tol).all()), (i, float(d.max()))
        assert mine.state[p]["step"] == int(ref.state[q]["step"])
        for k in ("exp_avg", "exp_avg_sq"):
            dm = (mine.state[p][k] - ref.state[q][k]).abs()
            r = ref.state[q][k].abs()   # moments: rounding of the larger earlier terms (per-tensor scale)
            assert bool((dm <= 1e-6 * r + 1e-6 * float(r.max())).all()), (i, k, float(dm.max()))


def test_adam_unaligned_scalar_path(cuda):
    """A parameter whose storage starts 4 B past a 16-B boundary takes the
    scalar lanes; results equal the aligned copy's bit for bit."""
    from pointnerf_amd.optim import Adam
    big = torch.randn(8193, device=cuda)
    p_un = torch.nn.Parameter(big[1:])            # view: storage offset 1 float
    p_al = torch.nn.Parameter(big[1:].clone())
    assert p_un.data_ptr() % 16 == 4 and p_al.data_ptr() % 16 == 0
    o1, o2 = Adam([p_un], lr=1e-3), Adam([p_al], lr=1e-3)
    for it in range(3):
        g = torch.randn(8192, device=cuda, generator=torch.Generator(device=cuda).manual_seed(it))
        p_un.grad, p_al.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    assert torch.equal(p_un.detach(), p_al.detach())


# One param group of 70 tensors: more than kAdamMax = 32, so the host launches three
# times with a fresh chunk table each; numels around 4 (the float4 quads), 1024 (one
# pass of the block), the 8192-element chunk and its multiples, and an empty tensor.
MANY_NUMELS = (1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 8196, 12287, 12288, 12289, 16384, 16385, 0)
MANY = 70


def _many_params(dev, seed):
    """Every fifth tensor is a view at storage offset 1 or 3 floats (the scalar lanes),
    the others start on a 16-B boundary: both kinds share each launch."""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i in range(MANY):
        n = MANY_NUMELS[i % len(MANY_NUMELS)]
        off = (1 if i % 10 == 4 else 3) if i % 5 == 4 else 0
        base = torch.randn(n + off, generator=g).to(dev)
        ps.append(torch.nn.Parameter(base[off:]))
        assert ps[-1].numel() == n and (n == 0 or ps[-1].data_ptr() % 16 == 4 * off)
    return ps


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_many_tensors_across_launches(cuda, wd):
    """A tensor's bits depend neither on its place in the chunk table nor on the launch
    it falls into: the group stepped at once equals every tensor stepped by an Adam of
    its own (single-tensor launches) bit for bit, and torch.optim.Adam under the bars
    of test_adam_matches_torch."""
    from pointnerf_amd.optim import Adam
    a = _many_params(cuda, 1)
    s = [torch.nn.Parameter(p.detach().clone()) for p in a]          # aligned copies, one optimizer each
    b = [torch.nn.Parameter(p.detach().clone()) for p in a if p.numel()]
    kept = [i for i, p in enumerate(a) if p.numel()]
    assert len(a) > 64 and sum(p.numel() == 0 for p in a) == 4
    assert sum(p.data_ptr() % 16 != 0 for p in a if p.numel()) == 14
    kw = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    mine, single = Adam(a, **kw), [Adam([p], **kw) for p in s]
    ref = torch.optim.Adam(b, foreach=False, fused=False, **kw)
    for it in range(6):
        gs = _grads(a, 100 + it)
        for i, g in enumerate(gs):
            a[i].grad, s[i].grad = g.clone(), g.clone()
        for j, i in enumerate(kept):
            b[j].grad = gs[i].clone()
        if it == 3:   # a parameter without a gradient this step: from here on it steps in a launch of its own
            a[9].grad = s[9].grad = b[kept.index(9)].grad = None
        mine.step()
        for o in single:
            o.step()
        ref.step()
    for i, (p, q) in enumerate(zip(a, s)):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), (i, p.numel())
        assert mine.state[p]["step"] == single[i].state[q]["step"] == (5 if i == 9 else 6)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(mine.state[p][k].view(torch.int32), single[i].state[q][k].view(torch.int32)), (i, k)
    for j, i in enumerate(kept):
        p, q = a[i], b[j]
        d = (p.detach() - q.detach()).abs()
        assert bool((d <= 1e-6 * q.detach().abs() + 1e-9).all()), (i, float(d.max()))
        assert mine.state[p]["step"] == int(ref.state[q]["step"])
        for k in ("exp_avg", "exp_avg_sq"):
            dm = (mine.state[p][k] - ref.state[q][k]).abs()
            r = ref.state[q][k].abs()
            assert bool((dm <= 1e-6 * r + 1e-6 * float(r.max())).all()), (i, k, float(dm.max()))


def test_adam_step_direct_edges(cuda):
    """n_tensors = 0 is a no-op that returns OK; step = 0 is refused before any launch."""
    import ctypes
    from pointnerf_amd import _lib as L
    st = L.stream_ptr(cuda)
    assert L.lib().pnr_adam_step(0, None, None, None, None, None, 5e-4, 0.9, 0.999, 1e-8, 0.0, 1, st) == L.PNR_OK
    p = torch.randn(8193, device=cuda)
    g, m, v = torch.randn(8193, device=cuda), torch.zeros(8193, device=cuda), torch.zeros(8193, device=cuda)
    keep = [t.clone() for t in (p, m, v)]
    tab = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in (p, g, m, v)]
    numel = (ctypes.c_int64 * 1)(8193)
    assert L.lib().pnr_adam_step(1, *tab, numel, 5e-4, 0.9, 0.999, 1e-8, 0.0, 0, st) == L.PNR_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((p, m, v), keep))
    assert L.lib().pnr_adam_step(1, *tab, numel, 5e-4, 0.9, 0.999, 1e-8, 0.0, 1, st) == L.PNR_OK
    torch.cuda.synchronize()
    assert not torch.equal(p, keep[0]) and bool(m.any()) and bool(v.any())


def test_adam_refuses_bad_params(cuda):
    from pointnerf_amd import _lib as L
    from pointnerf_amd.optim import Adam
    p = torch.nn.Parameter(torch.randn(8, 8, device=cuda).t())   # non-contiguous
    p.grad = torch.randn(8, 8, device=cuda)
    with pytest.raises(L.PnrError):
        Adam([p]).step()
