"""A plain `bench.py --gpus 1 --steps K --warmup W` does only what its headline needs: set-up, warm-up, the K timed steps and the
one JSON line, with at most 30 s of the whole run outside the steps.  Everything else it measures (per-kernel times and roofline,
the padded value layout, the CPU baseline, the other configurations) runs only under --full (tests/test_dist_gpu.py runs one)."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_unless_asked_for(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse_args().full is True


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    steps, warmup = 20, 5
    # a fresh process as the benchmark is run: no launcher variables, no test knobs of the library
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK") and not k.startswith("MSDA_")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=600, env=env)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    for key in ("kernels", "scatter_pass", "routes", "padded_value_layout", "other_configs"):
        assert key not in line, key
    rows = 16 * 6 * 300
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["query_rows_per_step"] == rows
    assert abs(line["value"] - rows / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * line["value"]
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    assert outside < 30.0, "%.1f s outside the steps (whole run %.1f s)" % (outside, wall)
