"""Every BASELINE config exactly as bench.py builds it, on the committed at-spec fixtures (tests/golden/spec_*.npz: windows over
the glass sphere's rim, text silhouettes, the pile of metallic-glass spheres, floor and wall penumbrae -- >= 3 000 pixels per
config, rendered offline with the threaded packet restatement of the oracle): hit ids and pixel indices exact, `t` bit-exact,
RGB within 1e-4, ray counters equal.  Under budget 0 and under bench.SCENE_BUDGET, the budget bench.py renders with: there
the semesterbild configs must build their per-cell candidate lists."""
import numpy as np
import pytest

import bench
from test_oracle_golden import SPEC_CASES, check_spec_window, make_spec_golden  # (test_oracle_golden puts tests/golden on the path)
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi
from test_parity_gpu import RGB_TOL, gpu_render

pytestmark = pytest.mark.gpu


def check_fixture(name, budget):
    meta, z = make_spec_golden.load(name)
    cfg, flat, _ = bench.build_workload(meta["workload"])
    worst, n_px = 0.0, 0
    for i, win in enumerate(meta["windows"]):
        argb, planes, st = gpu_render(cfg, flat, tuple(win), budget=budget)
        if budget and bench.WORKLOADS[meta["workload"]]["scene"] == "semesterbild":
            assert not st["notes"] & _abi.RT_NOTE_CELL_LISTS_OFF, st["notes"]
        worst = max(worst, check_spec_window(z, i, win, cfg, argb, planes, st, rgb_tol=RGB_TOL, want_stats=meta["stats"][i]))
        n_px += win[2] * win[3]
    print(f"{name} budget {budget}: {n_px} at-spec pixels, max |dRGB| vs the fixture {worst:.2e}")


@pytest.mark.parametrize("name", SPEC_CASES)
def test_gpu_reproduces_at_spec_fixture(name):
    """under the library's default budget (budget 0)"""
    check_fixture(name, 0)


@pytest.mark.parametrize("name", SPEC_CASES)
def test_gpu_reproduces_at_spec_fixture_under_the_bench_budget(name):
    """under bench.SCENE_BUDGET, the budget bench.py renders with: the per-cell candidate lists are built"""
    check_fixture(name, bench.SCENE_BUDGET)
