"""bench.py at N = 1 in its two modes: a plain run times the steps and prints the headline line; --full adds what takes runs of its
own (the CPU baseline, the secondary configs, the idle-queue enqueue probe).  32 clips x 48 frames (the size the switch tests of
tests/test_gpu_bench_path.py run), in fresh child processes."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "48"] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["M3T_SCAN_LOCK"] = "0"              # the pytest process may hold the persistent-scan ownership lock and is idle meanwhile
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (lines, out.stderr[-1500:])
    return json.loads(lines[0])


def test_plain_and_full_bench_lines():
    plain = _bench()
    assert plain["value"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1 and plain["config"]["frames"] == 48
    assert plain["cpu_baseline"] is None and plain["host_enqueue_ms_idle"] is None
    assert not {"aux", "aux_ms", "aux_ms_per_step", "speedup_vs_cpu", "cpu_baseline_error"} & set(plain)
    assert plain["roofline"] is not None and plain["kernels"]

    full = _bench("--full", "--cpu-clips", "2", "--aux", "c1", "--aux-budget", "300")
    assert full["value"] > 0 and full["cpu_baseline"]["value"] > 0 and full["speedup_vs_cpu"] > 0
    assert full["host_enqueue_ms_idle"] > 0
    assert "note" not in full["aux"] and full["aux"]["c1"]["ms_per_step"] > 0
    assert full["aux_ms"] == full["aux_ms_per_step"] == {"c1": full["aux"]["c1"]["ms_per_step"]}
    # the persistent-scan count covers the timed steps only, whatever runs after them
    assert full["persistent_scan_launches_per_step"] == plain["persistent_scan_launches_per_step"]
