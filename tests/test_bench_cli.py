"""bench.py's two kinds of run: a plain one measures the headline alone, `--full` adds the secondary workloads and the
CPU baselines (the parser on the host; one plain run end to end on the GPU)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _args(*argv):
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(list(argv))
    return a.with_secondary, a.with_cpu_baseline


def test_plain_run_leaves_out_what_full_adds():
    assert _args() == (False, False)
    assert _args("--gpus", "1", "--steps", "20", "--warmup", "5") == (False, False)
    assert _args("--no-secondary", "--no-cpu-baseline") == (False, False)
    assert _args("--full") == (True, True)
    assert _args("--full", "--no-secondary") == (False, True)
    assert _args("--full", "--no-cpu-baseline") == (True, False)
    assert _args("--full", "--no-secondary", "--no-cpu-baseline") == (False, False)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """One plain run (K = 100 as the headline, one timed step): ONE JSON line with the contract's fields and the roofline of
    the timed steps, no secondary workload and no CPU baseline; --dump-outputs still writes its files."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--workload", "k100",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[:2000]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "tasks/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 1000 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert set(d["roofline"]["per_kernel"]) <= {"k_mm_live", "k_mm_split"} and d["roofline"]["frac"] > 0
    assert "secondary" not in d and "cpu_baseline" not in d
    assert (tmp_path / "task_accuracies.npy").exists() and set(d["dumped_outputs"]["files"]) == set(os.listdir(tmp_path))
