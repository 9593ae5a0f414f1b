"""bench.py on one GPU at a small size: a plain run prints the headline line and leaves out what takes runs of its own; --full adds
the CPU baseline and the box's copy rate behind the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--rows-per-gpu", "20000", "--nnz-per-gpu", "300000"] + list(extra), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_leaves_out_what_full_measures(gpu):
    plain = _bench()
    full = _bench("--full", "--cpu-seconds", "1")
    for d in (plain, full):
        assert d["metric"] == "GloVe pair-updates/sec at dim=200" and d["unit"] == "pair-updates/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and (d["n_gpus"], d["steps"], d["warmup"]) == (1, 2, 1)
        # value and ms_per_step are the same timed region: every nonzero once per step
        assert d["value"] == pytest.approx(d["config"]["nnz_per_gpu"] * 1e3 / d["ms_per_step"], rel=1e-9)
        assert len(d["mean_cost_per_step"]) == 3 and d["roofline"]["kernel_ms"] > 0
    assert full["config"] == plain["config"]
    assert "cpu_baseline" not in plain and plain["roofline"]["box_copy_GBps"] is None
    cb = full["cpu_baseline"]
    assert cb["value"] > 0 and cb["single_thread"]["value"] > 0 and cb["kind"] == "port"
    assert full["roofline"]["box_copy_GBps"] > 0
