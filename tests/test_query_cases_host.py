"""The world-grid option matrix (tests/query_cases.py) under the oracle alone:
every case's claims (so no case passes while testing nothing), and the oracle
itself at the kernel and query sizes the shipped flag sets never reach --
oracle_knn against the brute-force statement of the searched shells, the
dilation against a numpy restatement of its window."""
import numpy as np
import pytest

import query_cases as QC
from oracle import oracle as O


@pytest.mark.parametrize("name", list(QC.CASES))
def test_case_claims(name):
    got = QC.claims(name)
    assert len(got) >= 2
    for what, value, ok in got:
        assert ok, f"{name}: {what} (measured {value})"


def test_table_is_the_option_matrix():
    """The rows the GPU file relies on: the dense cases are the eight K rows plus
    the two mixed kernels, and k377-K8 is a two-layer walk (kernel_size[0] = 3)."""
    assert len(QC.CASES) == 25 and len(QC.DENSE_CASES) == 9
    assert (QC.build("k377-K8")[0]["opt"].kernel_size[0] + 1) // 2 == 2
    for name, layers in (("q111-k111", 1), ("k555-K16", 3), ("k777-K32", 4), ("k999-K32", 5), ("k733-K8", 4)):
        assert (QC.build(name)[0]["opt"].kernel_size[0] + 1) // 2 == layers


@pytest.mark.parametrize("name", ["q111-k111", "k555-K16", "k777-K32", "k999-K32", "k733-K8", "flat-k5-K16"])
def test_oracle_knn_equals_bruteforce_sets(name):
    """As test_oracle_query.test_knn_equals_bruteforce_sets does at kernel 3: on
    150 seeded filled samples, as many neighbours as the searched shells hold (up
    to K) and the same sorted squared distances."""
    sc, xyz, ref = QC.build(name)
    loc, _, pidx = QC.filled(name)
    pick = np.sort(np.random.default_rng(5).choice(len(loc), size=150, replace=False))
    g, K = ref["grid"], sc["opt"].K
    bf = O.knn_bruteforce(xyz, loc[pick], g["hp"], sc["opt"], g)
    full = 0
    for want, got, p in zip(bf, pidx[pick], loc[pick]):
        got = got[got >= 0]
        k = min(len(want), K)
        assert len(got) == k and len(set(got.tolist())) == k
        full += len(want) > K
        wd = sorted(d for d, _ in want)[:k]
        gd = sorted(float(np.sum((xyz[i] - p) ** 2, dtype=np.float64)) for i in got)
        np.testing.assert_allclose(gd, wd, rtol=1e-5, atol=1e-12)
    if name in QC.DENSE_CASES:   # (a third or more of their samples fill all K slots: the claims)
        assert full > 10, "some samples must see more than K candidates (the replace phase)"


def _window_or(kept, qs):
    """Cell v is marked iff a kept voxel lies in [v - (qs+1)/2 + 1, v + qs/2] on each axis."""
    out = kept
    for axis in range(3):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for d in range(-((qs[axis] + 1) // 2) + 1, qs[axis] // 2 + 1):
            dst = [slice(None)] * 3
            src = [slice(None)] * 3
            dst[axis] = slice(max(0, -d), min(n, n - d))      # v
            src[axis] = slice(max(0, d), min(n, n + d))       # v + d
            acc[tuple(dst)] |= out[tuple(src)]
        out = acc
    return out


@pytest.mark.parametrize("name", ["q222", "q535", "aniso-k5-q542"])
def test_oracle_dilation_equals_window(name):
    sc, _, ref = QC.build(name)
    g = ref["grid"]
    dims = tuple(int(d) for d in g["hp"]["dims"])
    kept = (g["coor_2_occ"] >= 0).reshape(dims)
    want = _window_or(kept, [int(q) for q in sc["opt"].query_size])
    got = g["coor_occ"].reshape(dims) > 0
    assert kept.sum() > 1000 and want.sum() > kept.sum()
    assert np.array_equal(got, want)
