"""`python bench.py --gpus N` launches its own N ranks.

The driver's scaling run calls `python bench.py --gpus N` without torchrun; the
parent must start N rank processes (torch.distributed.run) before any GPU call,
wait for them and print ONE line carrying n_gpus = N and the process group's
world size.  --dry-run exercises that machinery on the CPU (gloo, no libpnr):
launcher, band shards, one all-gather per step, max-over-ranks timing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, extra=()):
    env = dict(os.environ, PNR_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3",
                        "--warmup", "1", "--dry-run", *extra], capture_output=True, text=True, env=env,
                       timeout=240, cwd=ROOT)
    return p


@pytest.mark.parametrize("n", [2, 3])
def test_bench_self_launches_n_ranks(n):
    p = _run(n)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == n and rec["rccl_world"] == n and rec["dist_backend"] == "gloo"
    assert rec["frames_equal"] is True
    assert len(rec["ms_per_step_per_rank"]) == n
    assert rec["ms_per_step"] == max(rec["ms_per_step_per_rank"])
    assert "torch.distributed.run" in rec["launcher"]


def test_bench_single_rank_dry_run_needs_no_launcher():
    p = _run(1)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads(p.stdout.strip())
    assert rec["n_gpus"] == 1 and "launcher" not in rec


def test_bench_dump_outputs_is_repeatable(tmp_path):
    """--dump-outputs DIR writes the last timed step's frames as float32 .npy
    files, a relative DIR taken from the caller's directory; two runs with the
    same arguments write the same bytes; --full is accepted and --steps is the
    number of timed steps."""
    import numpy as np
    recs = []
    for d in ("a", "b"):
        env = dict(os.environ, PNR_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
        env.pop("WORLD_SIZE", None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                            "--warmup", "1", "--dry-run", "--full", "--dump-outputs", d], capture_output=True,
                           text=True, env=env, timeout=240, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        recs.append(json.loads(p.stdout.strip()))
    assert all(r["steps"] == 2 and r["ms_per_step"] > 0 for r in recs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frame0_ray_color.npy"] == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape == (64 * 64, 4) and np.isfinite(a).all()
        assert np.array_equal(a, b)


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path, monkeypatch):
    """An output larger than its share of the budget is written for a seeded
    sample of its rows: the same rows of every array of the group, listed in
    rays.npy, all files together within the budget."""
    import numpy as np
    import torch
    monkeypatch.syspath_prepend(ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    R = 20000
    g = torch.Generator().manual_seed(0)
    arrays = {"ray_color": torch.randn(R, 128, generator=g), "opacity": torch.randn(R, 80, generator=g),
              "ray_mask": (torch.rand(R, generator=g) > 0.5).to(torch.int8)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("", arrays)])
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= 1 << 20
    rows = got.pop("rays")
    assert rows.dtype == np.float64 and 1000 < len(rows) < R and np.all(np.diff(rows) > 0)
    for k, v in arrays.items():
        assert got[k].dtype == np.float32
        assert np.array_equal(got[k], v.numpy()[rows.astype(np.int64)].astype(np.float32))
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
    # a small group is written whole, without a row list
    bench.dump_outputs(str(tmp_path / "c"), [("x_", {"loss": torch.tensor([1.5])})])
    assert os.listdir(tmp_path / "c") == ["x_loss.npy"]


def test_bench_launcher_reports_a_failing_rank():
    # an unknown flag makes every rank exit 2: the parent must exit non-zero, print no line
    env = dict(os.environ, PNR_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=dict(env, PNR_BENCH_FAIL_RANK="1"), timeout=240, cwd=ROOT)
    assert p.returncode != 0
    assert p.stdout.strip() == ""
    assert "exited" in p.stderr
