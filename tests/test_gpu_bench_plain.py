"""A plain bench.py run (--gpus 1 --steps K --warmup W): the line's headline fields, nothing measured beside them
(no CPU baseline, no `pipelined` steps: those are --full's), and --dump-outputs: the last timed step's hit records,
equal to an in-process cast of the same frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(rt, depth12, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "rays/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and "depth-12" in d["metric"]
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - 1920 * 1080 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]  # (both rounded on the line)
    assert d["cpu_baseline"] is None and "pipelined" not in d
    assert d["roofline"]["rays_per_launch"] == 1920 * 1080
    files = sorted(os.listdir(out))
    assert files == ["info.npy", "pos_steps.npy", "t.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 1000 * 1000
    ref = depth12.cast_frame((4.0, 90.0, 4.0), rt.normalize([1.0, -0.45, 1.0]), 1920, 1080, 16384)
    for k in ("pos_steps", "t", "info"):
        got = np.load(out / (k + ".npy"))
        assert got.dtype in (np.float32, np.float64)
        want = ref[k].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.astype(want.dtype).view(np.uint32), want.view(np.uint32)), k
