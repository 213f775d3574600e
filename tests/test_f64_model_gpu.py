"""The GPU against the independent float64 model (tests/f64_model.py), with the same intervals and TOL as the CPU
checks in test_f64_model_soft_shadows.py: the synthetic config-3 / config-4 scenes full frame on the fused path, the
phase-split path and (config 4) the chained level schedule; the at-spec config-3 windows as bench.build_workload makes
them, under budget 0 and under bench.SCENE_BUDGET (where the per-cell candidate lists must really be built)."""
import pytest

import bench
import f64_cases as fc
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi
from test_parity_gpu import gpu_render

pytestmark = pytest.mark.gpu

STATS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written")
FORMS = {"fused": {}, "split": dict(phases=_abi.RT_PHASES_SPLIT), "chained": dict(levels=_abi.RT_LEVELS_CHAINED)}


@pytest.mark.parametrize("key", sorted(fc.SYN_CASES))
def test_gpu_synthetic_scene_within_the_float64_intervals(key):
    cfg, flat = fc.syn_workload(key)
    res, want = fc.syn_intervals(key), fc.model_counts(key)
    forms = ["fused", "split"] + (["chained"] if key.startswith("c4") else [])
    for form in forms:
        argb, planes, st = gpu_render(cfg, flat, None, **FORMS[form])
        s = fc.check(res, cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
        fc.assert_guards(f"gpu {key} {form}", s)
        assert not s["bad"], (form, s["bad"][:5])
        assert {k: st[k] for k in STATS} == want, form


@pytest.mark.parametrize("budget", [0, bench.SCENE_BUDGET], ids=["budget0", "scene_budget"])
@pytest.mark.parametrize("name", fc.SPEC_NAMES)
def test_gpu_at_spec_windows_within_the_float64_intervals(name, budget):
    cfg, flat, meta, z = fc.spec_workload(name)
    res = fc.spec_intervals(name)
    for win in meta["windows"]:
        argb, planes, st = gpu_render(cfg, flat, tuple(win), budget=budget)
        if budget:
            assert not st["notes"] & _abi.RT_NOTE_CELL_LISTS_OFF, st["notes"]
        x0, y0, w, h = win
        mine = [r for r in res if x0 <= r["px"][0] < x0 + w and y0 <= r["px"][1] < y0 + h]
        s = fc.check(mine, cfg.width, planes["rgb"], planes["hit_id"], planes["hit_t"], t_rel=1e-5)
        print(f"gpu {name} budget {budget} window {win}: worst {s['worst']:.2e}, ambiguous {s['ambiguous']}")
        assert not s["bad"], (win, s["bad"][:5])
