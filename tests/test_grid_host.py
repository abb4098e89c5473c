"""The grid's host layer without a GPU: what GridHandle.build
hands to libpnr for each flag set -- the entry points in order, the pnr_grid_spec
and pnr_grid_params bytes, the host dict -- pinned by tests/golden/grid_host.json,
which `python tests/test_grid_host.py` recorded on the tree before the host layer
was rebuilt; the rebuild key; the refusals that need no device.

The library is replaced by a recorder (_FakeLib), so GridHandle.build itself runs:
nothing here depends on how querier.py arranges the work inside it."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_host.json")
BBOX = np.array([-0.31, -0.52, -0.2, 0.3, 0.55, 0.93], np.float32)   # the fixed bbox of every host build
N_POINTS = 1000


def _opts():
    from pointnerf_amd.options import FLAGSETS, flagset_opt, lego_opt
    cases = {name: flagset_opt(name) for name in FLAGSETS}
    cases["no_ranges"] = lego_opt(ranges=[1, 1, 1, 0, 0, 0])   # min >= max: unset (qpiw.py:61-62)
    cases["host_bbox"] = lego_opt(grid_host_bbox=True)
    cases["grow"] = lego_opt(max_o_policy="grow", max_o=500)   # N_POINTS > max_o, 700 occupied voxels
    return cases


class _FakeLib:
    """libpnr.so's grid entry points as a recorder: (name, bytes of the struct
    argument) per call.  pnr_points_bbox answers BBOX, pnr_grid_stats_get
    n_voxels = 700 and dims = (3, 4, 5)."""

    def __init__(self):
        self.calls = []

    def names(self):
        return [c[0] for c in self.calls]

    def pnr_last_error(self):
        return b"fake"

    def pnr_create(self, device, out):
        out._obj.value = 1
        return 0

    def pnr_destroy(self, h):
        return 0

    def pnr_points_bbox(self, xyz, n, out, stream):
        self.calls.append(("pnr_points_bbox", b""))
        ctypes.memmove(out, BBOX.ctypes.data, BBOX.nbytes)
        return 0

    def pnr_grid_build(self, h, xyz, n, gp, stream):
        self.calls.append(("pnr_grid_build", bytes(gp._obj)))
        return 0

    def pnr_grid_build_dev(self, h, xyz, n, sp, stream):
        self.calls.append(("pnr_grid_build_dev", bytes(sp._obj)))
        return 0

    def pnr_grid_stats_get(self, h, out):
        self.calls.append(("pnr_grid_stats_get", b""))
        out._obj.n_voxels = 700
        out._obj.dims[:] = [3, 4, 5]
        return 0


@pytest.fixture
def fake(monkeypatch):
    """(lib, make): the recorder in place of the library, and GridHandle
    factories whose handles are closed before the real library is back."""
    from pointnerf_amd import _lib as L
    from pointnerf_amd import querier as Q
    lib = _FakeLib()
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(L, "require_gpu", lambda t=None: None)
    monkeypatch.setattr(L, "stream_ptr", lambda device=None: None)
    made = []

    def make():
        made.append(Q.GridHandle(torch.device("cpu")))
        return made[-1]

    yield lib, make
    for g in made:
        g.close()


def _xyz():
    return torch.zeros(N_POINTS, 3)


def _enc(v):
    if isinstance(v, np.ndarray) or isinstance(v, np.generic):
        a = np.asarray(v)
        return {"dtype": str(a.dtype), "shape": list(a.shape), "hex": a.tobytes().hex()}
    return v


def _observe(make, lib, opt):
    """What one build of opt does, as the fixture holds it."""
    from pointnerf_amd.querier import grid_spec
    sp, base = grid_spec(opt)
    g = make()
    first = len(lib.calls)
    hp = g.build(opt, _xyz())
    calls = lib.calls[first:]
    names = [c[0] for c in calls]
    out = {"calls": names, "path": "dev" if "pnr_grid_build_dev" in names else "host",
           "structs": [c[1].hex() for c in calls if c[1]],
           "spec": None if sp is None else bytes(sp).hex(),
           "dims_max": None if sp is None else list(sp.dims_max),
           "base": None if base is None else {k: _enc(base[k]) for k in sorted(base)},
           "hp_type": type(hp).__name__,
           "hp": {k: _enc(dict.__getitem__(hp, k)) for k in sorted(dict.keys(hp))}}
    # pnr_grid_params for the fixed bbox, whichever path the flag set itself takes
    host = SimpleNamespace(**{**vars(opt), "grid_host_bbox": True, "max_o_policy": "reservoir"})
    first = len(lib.calls)
    make().build(host, _xyz())
    out["params"] = [c[1].hex() for c in lib.calls[first:] if c[0] == "pnr_grid_build"][0]
    return out


def _observe_all(make, lib):
    return {name: _observe(make, lib, opt) for name, opt in _opts().items()}


def test_build_hands_libpnr_what_the_fixture_recorded(fake):
    lib, make = fake
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(_observe_all(make, lib)))
    assert sorted(got) == sorted(want)
    for name in want:
        for k in want[name]:
            assert got[name][k] == want[name][k], (name, k)


def test_fixture_shows_the_paths_the_flag_sets_take():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["lego"]["dims_max"] == [163, 290, 189] and want["lego"]["path"] == "dev"
    d = want["scene101"]["dims_max"]
    assert d[0] * d[1] * d[2] == 1971935064 > 1 << 28 and want["scene101"]["path"] == "host"
    assert want["scene101"]["calls"] == ["pnr_points_bbox", "pnr_grid_build"]
    assert [want[k]["path"] for k in ("ship", "truck", "no_ranges", "host_bbox")] == ["dev", "dev", "host", "host"]
    assert want["no_ranges"]["spec"] is None and want["host_bbox"]["spec"] is not None
    assert want["lego"]["hp_type"] == "GridHP" and want["host_bbox"]["hp_type"] == "dict"
    # grow: the host build, the voxel count, the build again with max_o raised to it
    assert want["grow"]["calls"] == ["pnr_points_bbox", "pnr_grid_build", "pnr_grid_stats_get", "pnr_grid_build"]


KEY_FIELDS = dict(vsize=[0.005, 0.004, 0.004], vscale=[2, 2, 3], kernel_size=[5, 3, 3], query_size=[3, 3, 5],
                  ranges=[-0.638, -1.141, -0.346, 0.634, 1.149, 1.142], max_o=830001, P=10, slot0_drop=0,
                  grid_seed=1, max_o_policy="grow")


@pytest.mark.parametrize("field", sorted(KEY_FIELDS))
def test_key_differs_when_one_grid_field_does(fake, field):
    from pointnerf_amd.options import lego_opt
    lib, make = fake
    g, xyz = make(), _xyz()
    g.build(lego_opt(), xyz)
    k0, n0 = g.key, len(lib.calls)
    g.build(lego_opt(), xyz)                     # an equal opt: the same key, nothing rebuilt
    assert g.key == k0 and len(lib.calls) == n0
    g.build(lego_opt(**{field: KEY_FIELDS[field]}), xyz)
    assert g.key != k0 and len(lib.calls) > n0


@pytest.mark.parametrize("field,value", [("grid_host_bbox", True), ("grid_dev_max_cells", 1000),
                                         ("radius_limit_scale", 3.0), ("depth_limit_scale", 1.0)])
def test_key_covers_the_options_that_choose_the_path_and_the_hp(fake, field, value):
    """New with the GridOpts key: these four decide the path or the returned hp
    and were not in the key before (an opt that changed only them got the cached hp)."""
    from pointnerf_amd.options import lego_opt
    lib, make = fake
    g, xyz = make(), _xyz()
    g.build(lego_opt(), xyz)
    k0 = g.key
    g.build(lego_opt(**{field: value}), xyz)
    assert g.key != k0


def test_key_point_half(fake):
    from pointnerf_amd.options import lego_opt
    lib, make = fake
    g, xyz = make(), _xyz()
    g.build(lego_opt(), xyz)
    k0, n0 = g.key, len(lib.calls)
    xyz.add_(1.0)                                # in place: the version counter moves
    g.build(lego_opt(), xyz)
    assert g.key != k0 and len(lib.calls) > n0
    k1 = g.key
    g.build(lego_opt(), xyz[:500])
    assert g.key != k1


def test_max_o_policy_refusal(fake):
    from pointnerf_amd._lib import PnrError
    from pointnerf_amd.options import lego_opt
    lib, make = fake
    with pytest.raises(PnrError, match="max_o_policy 'fifo'"):
        make().build(lego_opt(max_o_policy="fifo"), _xyz())
    assert lib.names() == []


def test_unset_ranges_build_on_the_host(fake):
    """opt.ranges = None is 'unset' like min >= max (grid_spec and
    hyperparameters_from_bbox say so): the build takes the host path."""
    from pointnerf_amd.options import lego_opt
    lib, make = fake
    hp = make().build(lego_opt(ranges=None), _xyz())
    assert lib.names() == ["pnr_points_bbox", "pnr_grid_build"] and type(hp) is dict


def test_table_bytes_est_sums_the_layout_terms(fake):
    """stats()["table_bytes_est"] from the per-cell sizes GridLayout allocates
    (csrc/grid_tables.h): three int32 cell tables; per 32-cell word 68 B of
    cell_bytes (32 occupancy + 32 held + a 4-B word rank), the 4-B bitmap word,
    the 8-B query word and its 4-B count; one 4-B coarse-map word per 8 x 32
    (z, y) block of cells."""
    from pointnerf_amd.options import lego_opt
    from pointnerf_amd.querier import GRID_BYTES_PER_CELL
    per_cell = 3 * 4 + (68 + 4 + 8 + 4) / 32 + 4 / (8 * 32)
    assert GRID_BYTES_PER_CELL == per_cell
    lib, make = fake
    g = make()
    g.build(lego_opt(), _xyz())
    st = g.stats()
    assert st["table_cells"] == 60 and st["table_bytes_est"] == int(60 * per_cell) == 878


def test_null_pointer_refusals_need_no_device():
    from pointnerf_amd import _lib as L
    lib = L.lib()

    def refused(rc, message):
        assert rc == L.PNR_EINVAL
        assert lib.pnr_last_error().decode() == message

    refused(lib.pnr_grid_build(None, None, 0, None, None), "grid_build: null pointer")
    refused(lib.pnr_grid_build_dev(None, None, 0, None, None), "grid_build_dev: null pointer")
    refused(lib.pnr_query(None, None, None, None, None), "query: null pointer")
    refused(lib.pnr_grid_stats_get(None, None), "grid_stats: null pointer")
    refused(lib.pnr_grid_geometry(None, None, None, None), "grid_geometry: grid not built")
    refused(lib.pnr_grid_bbox(None, None), "grid_bbox: null pointer")
    refused(lib.pnr_grid_export(None, None, None, None, None, None), "grid_export: grid not built")


if __name__ == "__main__":   # record the fixture (run on the tree whose behaviour is to be kept)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pointnerf_amd import _lib as L
    from pointnerf_amd import querier as Q
    lib = _FakeLib()
    L.lib, L.require_gpu, L.stream_ptr = (lambda: lib), (lambda t=None: None), (lambda device=None: None)
    handles = []

    def make():
        handles.append(Q.GridHandle(torch.device("cpu")))
        return handles[-1]

    obs = _observe_all(make, lib)
    for g in handles:
        g.close()
    with open(GOLDEN, "w") as f:
        json.dump(obs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: " + ", ".join(f"{k} -> {v['path']}" for k, v in obs.items()))
