"""bench.py --dump-outputs: what the last timed step returned, in files -- the step's RMSDs (the same numbers --dump-rmsd writes for
that step), its status codes, and the fitted coordinates of a seeded sample of its frames; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    K, B, n = 3, 64, 200000
    out, rmsd = tmp_path / "out", tmp_path / "rmsd.npy"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--atoms", str(n), "--steps", str(K), "--warmup", "1", "--frames-per-step", str(B),
           "--dump-outputs", str(out), "--dump-rmsd", str(rmsd)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    line = json.loads(lines[0])
    assert line["steps"] == K and len(line["config"]["step_ms"]) == K and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and line["roofline"]["copy_floor_live"] is None       # a plain run: no --full figures
    got = {f: np.load(out / (f + ".npy")) for f in ("rmsd", "status", "fitted_positions")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["rmsd"], np.load(rmsd)[(K - 1) * B:]) and np.isfinite(got["rmsd"]).all()
    assert got["status"].shape == (B,) and (got["status"] == 0).all()
    assert got["fitted_positions"].shape == (4, n, 3) and np.isfinite(got["fitted_positions"]).all()
    assert sum(os.path.getsize(out / (f + ".npy")) for f in got) <= 64 << 20
