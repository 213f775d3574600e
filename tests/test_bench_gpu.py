"""bench.py as its callers run it, in a process of its own: a plain run prints the headline line and dumps the last timed
frame, and nothing else; --full adds the figures that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("ms_per_frame_alone", "value_alone", "roofline", "d2h_ms", "boundary", "lean_scene", "other_workloads",
             "cpu_baseline")


def run_bench(*args, timeout):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py"), *args]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return json.loads(proc.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_frame(tmp_path):
    line = run_bench("--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path), timeout=300)
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("Mray/s") and line["steps"] == 4 and line["warmup"] == 2
    assert line["value"] == pytest.approx(line["config"]["rays_per_frame"] / line["ms_per_step"] / 1e3)
    assert line["config"]["rays_per_frame"] == 1620 * 1350 * 16
    assert [k for k in FULL_ONLY if k in line] == []
    assert line["outputs"] == {"frame": [1350, 1620, 4]}
    frame = np.load(tmp_path / "frame.npy")
    assert frame.shape == (1350, 1620, 4) and frame.dtype == np.float32 and frame.any()


@pytest.mark.gpu
def test_full_run_adds_the_frame_alone_and_the_roofline():
    line = run_bench("--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-other-workloads", timeout=600)
    assert [k for k in FULL_ONLY if k not in line] == ["other_workloads", "cpu_baseline"]
    assert line["ms_per_frame_alone"] > 0 and line["roofline"]["kernel_ms"] == line["ranks"][0]["kernel_ms"] > 0
    assert line["roofline"]["kernel_ms_note"].startswith("mean of 4 launches")
