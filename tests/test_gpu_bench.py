"""`-m gpu`: bench.py end to end on a small frame.  A plain run prints the headline and what its timed region recorded;
the side measurements (runs of their own, the CPU baseline) wait for --full."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("value_spread", "roofline_quarter", "gate", "fp16_storage", "correlation", "shared_window", "best_schedule",
             "as_called", "two_streams", "cpu_baseline", "parity", "four_branches")


def _plain_run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
                       + list(extra), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("extra", [("--height", "256", "--width", "448"), ("--workload", "vimeo64")], ids=["slowmo", "vimeo64"])
def test_plain_bench_run_is_the_headline_alone(extra):
    res = _plain_run(*extra)
    assert all(k in res for k in HEADLINE), sorted(res)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["value"] > 0 and res["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in res]
    if extra[0] == "--height":
        assert res["roofline"]["launches_timed"] == 2 * 6      # the timed region's own events: six C=196 warps per step
