"""World-grid query option matrix (inputs only, no GPU): named cases off the
shipped flag sets -- query sizes 1..7 and mixed, kernel sizes 1..9 and mixed,
K 1..32 on the generic walk, the radius test off, anisotropic voxels, a cloud
crossing ranges, flat clouds -- each with the oracle's result and the claims
that keep the case from passing while testing nothing.

build(name) -> (sc, xyz, ref) is cached, so test_query_cases_host.py (the
claims, the oracle against brute force) and test_gpu_query_options.py (the
kernels against the oracle) share one oracle run per case.  Nothing here may
be modified by a test."""
import functools

import numpy as np

from oracle import oracle as O
from scenes import scene

F32 = np.float32
DEFAULTS = dict(n_points=20000, H=32, W=32, theta=70.0)
DENSE = dict(n_points=200000, P=26, H=24, W=24, radius_limit_scale=0.0)
ANISO = dict(vsize=[0.005, 0.004, 0.003], vscale=[1, 2, 3])


def flat(x):
    """The cloud pressed onto the plane z = 0.3."""
    return (x * np.array([1, 1, 0], F32) + np.array([0, 0, 0.3], F32)).astype(F32)


def _k(n):
    return [n, n, n]


CASES = {
    "base": dict(),
    "q111-k111": dict(query_size=_k(1), kernel_size=_k(1), H=64, W=64),
    "q222": dict(query_size=_k(2)),
    "q535": dict(query_size=[5, 3, 5]),
    "q353": dict(query_size=[3, 5, 3]),
    "q444-k555": dict(query_size=_k(4), kernel_size=_k(5)),
    "q777-k777": dict(query_size=_k(7), kernel_size=_k(7), radius_limit_scale=0.0),
    "k555-K1": dict(DENSE, kernel_size=_k(5), K=1),
    "k555-K8": dict(DENSE, kernel_size=_k(5), K=8),
    "k555-K16": dict(DENSE, kernel_size=_k(5), K=16),
    "k555-K32": dict(DENSE, kernel_size=_k(5), K=32),
    "k777-K8": dict(DENSE, kernel_size=_k(7), K=8),
    "k777-K16": dict(DENSE, kernel_size=_k(7), K=16),
    "k777-K32": dict(DENSE, kernel_size=_k(7), K=32),
    "k733-K8": dict(DENSE, kernel_size=[7, 3, 3], K=8),
    "k377-K8": dict(DENSE, kernel_size=[3, 7, 7], K=8),      # the 3x3x3 kernel on a wider pad
    "k999-K32": dict(kernel_size=_k(9), K=32, radius_limit_scale=0.0),
    "r0": dict(radius_limit_scale=0.0),
    "r1.5": dict(radius_limit_scale=1.5),
    "aniso": dict(ANISO),
    "aniso-k5-q542": dict(ANISO, kernel_size=_k(5), query_size=[5, 4, 2], radius_limit_scale=0.0),
    "clipped": dict(ranges=[-0.3, -0.5, -0.1, 0.3, 0.6, 0.5], H=64, W=64),
    "flat-k1": dict(xform=flat, kernel_size=_k(1), query_size=_k(1), H=64, W=64),
    "flat-k3": dict(xform=flat),
    "flat-k5-K16": dict(xform=flat, kernel_size=_k(5), query_size=_k(5), K=16, radius_limit_scale=0.0),
}
DENSE_CASES = [n for n, c in CASES.items() if c.get("n_points") == DENSE["n_points"]]
FLAT_DIMS_Z = {"flat-k1": 2, "flat-k3": 3, "flat-k5-K16": 6}


@functools.lru_cache(maxsize=None)
def build(name):
    """(sc, xyz, ref): the scene (tests/scenes.py, sc["xyz"] the transformed
    cloud), its cloud and the oracle's query of it."""
    over = dict(DEFAULTS, **CASES[name])
    xform = over.pop("xform", None)
    sc = scene(**over)
    xyz = np.ascontiguousarray(sc["xyz"] if xform is None else xform(sc["xyz"]), dtype=F32)
    sc["xyz"] = xyz
    ref = O.query_points(sc["opt"], xyz, sc["campos"], sc["camrot"], sc["raydir"], near=2.0, far=6.0)
    return sc, xyz, ref


# ------------------------------------------------------------------ measures
def filled(name):
    """(loc [S,3] world position, cell [S,3], pidx [S,K]) of the filled samples, ray-major."""
    sc, _, ref = build(name)
    hp = ref["grid"]["hp"]
    nf = ref["n_filled"]
    m = np.arange(sc["opt"].SR)[None, :] < nf[:, None]
    rp = O.raypos(sc["campos"], sc["raydir"], ref["mid_t"])
    rows = np.nonzero(m)
    loc = np.ascontiguousarray(rp[rows[0], ref["slot_d"][m]])
    cell = np.floor((loc - hp["shift"]) / hp["vsize_s"]).astype(np.int64)
    return loc, cell, ref["pidx_dense"][m]


def n_face(name):
    """Filled samples whose cell lies on a face of the grid."""
    _, cell, _ = filled(name)
    dims = build(name)[2]["grid"]["hp"]["dims"]
    return int(np.any((cell == 0) | (cell == dims - 1), axis=1).sum())


def n_dropped(name):
    """Points outside the case's grid."""
    _, xyz, ref = build(name)
    hp = ref["grid"]["hp"]
    c = np.floor((xyz - hp["shift"]) / hp["vsize_s"]).astype(np.int64)
    return int((~np.all((c >= 0) & (c < hp["dims"]), axis=1)).sum())


def rays_nfilled_differ(a, b):
    return int((build(a)[2]["n_filled"] != build(b)[2]["n_filled"]).sum())


def samples_compared(a, b):
    """(same, differ): the filled samples of the rays both cases fill alike (the
    same candidates), split by whether their neighbour rows are equal."""
    ra, rb = build(a)[2], build(b)[2]
    SR = ra["slot_d"].shape[1]
    m = np.arange(SR)[None, :] < ra["n_filled"][:, None]
    alike = (ra["n_filled"] == rb["n_filled"]) & np.all((ra["slot_d"] == rb["slot_d"]) | ~m, axis=1)
    m &= alike[:, None]
    K = min(ra["pidx_dense"].shape[2], rb["pidx_dense"].shape[2])
    eq = np.all(ra["pidx_dense"][m][:, :K] == rb["pidx_dense"][m][:, :K], axis=1)
    return int(eq.sum()), int((~eq).sum())


def n_full(name):
    """Filled samples with all K slots taken."""
    return int((build(name)[2]["pidx_dense"][..., -1] >= 0).sum())


# -------------------------------------------------------------------- claims
def claims(name):
    """[(what, measured, holds)] of one case, under the oracle alone.  The bounds
    are about half of what the reference measures."""
    sc, xyz, ref = build(name)
    out = []

    def claim(what, value, ok):
        out.append((what, value, bool(ok)))

    nf = ref["n_filled"]
    claim("valid rays >= 150", int(ref["ray_mask"].sum()), ref["ray_mask"].sum() >= 150)
    claim("filled samples >= 300", int(nf.sum()), nf.sum() >= 300)
    if name in ("q222", "q535", "q353"):
        v = rays_nfilled_differ(name, "base")
        claim("n_filled differs from base on >= 200 rays", v, v >= 200)
    if name == "q353":
        v = rays_nfilled_differ(name, "q535")
        claim("n_filled differs from q535 on >= 200 rays", v, v >= 200)
    if name in ("r0", "r1.5"):
        v = samples_compared(name, "base")[1]
        claim("pidx differs from base on >= 250 samples", v, v >= 250)
    if name in DENSE_CASES and sc["opt"].K >= 16:
        v = n_full(name)
        claim("samples with all K slots filled >= 200", v, v >= 200)
    if name == "k555-K1":
        _, _, p = filled(name)
        claim("every filled sample has a neighbour", int((p[:, 0] >= 0).sum()), np.all(p[:, 0] >= 0))
    if name.startswith("k777-K"):
        v = samples_compared(name, name.replace("k777", "k555"))[1]
        claim("differs from k555 on >= 350 samples", v, v >= 350)
    if name == "k733-K8":
        other = build("k777-K8")[2]["grid"]["hp"]["dims"]
        dims = ref["grid"]["hp"]["dims"]
        claim("dims differ from k777-K8's", (dims.tolist(), other.tolist()), not np.array_equal(dims, other))
        v = samples_compared(name, "k777-K8")[0]
        claim("same neighbours as k777-K8 on >= 4000 samples", v, v >= 4000)
    if name == "clipped":
        v = n_dropped(name)
        claim("points outside the grid >= 10000", v, v >= 10000)
        v = n_face(name)
        claim("filled samples in face cells >= 30", v, v >= 30)
    if name in FLAT_DIMS_Z:
        dz = int(ref["grid"]["hp"]["dims"][2])
        claim(f"dims[2] == {FLAT_DIMS_Z[name]}", dz, dz == FLAT_DIMS_Z[name])
        v = n_face(name)
        claim("filled samples in face cells >= 150", v, v >= 150)
    return out
