"""bench.py on the GPU at a small size: a plain run prints the result line from
the timed steps alone (nothing that needs runs of its own), and --dump-outputs
writes the last timed step's render_rays outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("grid_build", "stages_ms_isolated", "stage_rooflines", "cpu_baseline", "accuracy", "train")


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, cuda):
    H, SR, C = 48, 80, 128
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--hw", str(H), "--points", "20000", "--dump-outputs", "out"], capture_output=True, text=True,
                       env=env, timeout=240, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "Mray-samples/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "fp32h2" and rec["ms_per_step"] > 0
    # value is H*W*SR ray-samples per step over the step time
    assert rec["value"] == pytest.approx(H * H * SR / (rec["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert len(rec["per_step"]["valid_pairs"]) == 3
    assert not [k for k in FULL_ONLY if k in rec]
    out = tmp_path / "out"
    shapes = {"ray_color": (H * H, C), "opacity": (H * H, SR), "is_bg": (H * H,), "ray_mask": (H * H,)}
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in shapes)   # small enough: written whole
    got = {k: np.load(out / f"{k}.npy") for k in shapes}
    for k, s in shapes.items():
        assert got[k].dtype == np.float32 and got[k].shape == s and np.isfinite(got[k]).all(), k
    hit = got["ray_mask"] > 0
    assert 50 < hit.sum() < H * H and set(np.unique(got["ray_mask"])) <= {0.0, 1.0}
    # rays that hit nothing carry the background colour; rays that hit differ from it somewhere
    bg = np.random.default_rng(1).uniform(size=C).astype(np.float32)
    assert np.array_equal(got["ray_color"][~hit], np.broadcast_to(bg, ((~hit).sum(), C)))
    assert (np.abs(got["ray_color"][hit] - bg).max(axis=1) > 0).any()
