"""A frame rendered by the primary kernel compiled for its configuration (rt_primary_soft*_kernel) is, bit for bit, the frame
rt_primary_kernel renders: the specialised kernels only drop tests whose outcome the host already knows.

The config-3 frame (semesterbild, 1620x1350, anti-aliasing, soft shadows, text.obj) at full size and one ragged window,
with 10 and with 19 samples per light, under the library's default scene budget (receiver flags) and under 2 GiB (flags and
per-cell candidate lists): once as the library renders it and once with RT_PRIMARY_GENERIC=1.  That switch is read once
per process, so every render runs in a child process of its own, started before any GPU call, under its own time limit;
the first child that fails ends the test.  The parent compares what the children wrote: packed pixels, the aux float
planes, the ray counters -- and, from RT_TRACE_LAUNCHES, that each child really ran the kernel it was meant to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FEATURES = {10: ["high_resolution", "anti_aliasing", "soft_shadows"],  # bench.py's c3
            19: ["high_resolution", "high_quality"]}                   # the same frame with high_quality's 19 samples
BUDGETS = {"default": 0, "2GiB": 2 << 30}
WINDOWS = {"full": None, "ragged": (611, 397, 203, 117)}  # (x0, y0, w, h): no multiple of a 4x4 tile or a 16x16 super-tile
COUNTERS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written", "rays_traced")
CHILD_TIMEOUT_S = 240


def child(out_dir, n, budget):
    """One process = one value of RT_PRIMARY_GENERIC: renders both windows and writes them to out_dir."""
    sys.path.insert(0, ROOT)
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import ImageBuffer, RaytracerRenderer

    cfg = RenderConfig.from_features(FEATURES[n])
    assert cfg.point_light_multiplicator == n and not cfg.has("reflections") and not cfg.has("refractions")
    flat = scenes.semesterbild(cfg, "text").flatten()
    r = RaytracerRenderer(cfg, device=0, scene_budget=BUDGETS[budget])
    stats = {}
    for wname, win in WINDOWS.items():
        buf = ImageBuffer.new(cfg.width, cfg.height)
        planes = r.render(buf, flat, window=win, aux=True)
        np.savez(os.path.join(out_dir, wname + ".npz"), argb=np.asarray(buf.buffer), rgb=planes["rgb"], hit_id=planes["hit_id"],
                 hit_t=planes["hit_t"])
        stats[wname] = {k: int(r.last_stats[k]) for k in COUNTERS}
    with open(os.path.join(out_dir, "stats.json"), "w") as fh:
        json.dump(stats, fh)


def run_child(tmp_path, n, budget, generic):
    out = tmp_path / f"n{n}_{budget}_{'generic' if generic else 'default'}"
    out.mkdir()
    env = dict(os.environ, RT_TRACE_LAUNCHES="1")
    env.pop("RT_PRIMARY_GENERIC", None)
    if generic:
        env["RT_PRIMARY_GENERIC"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(out), str(n), budget]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert proc.returncode == 0, (cmd, proc.returncode, proc.stderr[-4000:])
    return out, proc.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("n", sorted(FEATURES))
def test_specialised_kernel_renders_the_generic_kernels_frame(tmp_path, n, budget):
    spec_dir, spec_log = run_child(tmp_path, n, budget, generic=False)
    gen_dir, gen_log = run_child(tmp_path, n, budget, generic=True)
    # which kernel each child ran (the launch label names it)
    expected = f"rt_primary_soft{n}_kernel" if budget == "2GiB" else f"rt_primary_soft{n}_flags_kernel"
    assert spec_log.count(expected + ": workgroups") == len(WINDOWS), spec_log[-2000:]
    assert "rt_primary_soft" not in gen_log and gen_log.count("rt_primary_kernel: workgroups") == len(WINDOWS), gen_log[-2000:]
    spec_stats, gen_stats = (json.load(open(d / "stats.json")) for d in (spec_dir, gen_dir))
    for wname in WINDOWS:
        a, b = np.load(spec_dir / (wname + ".npz")), np.load(gen_dir / (wname + ".npz"))
        assert b["argb"].any() and (b["hit_id"] >= 0).any(), wname  # (a frame was rendered at all)
        for plane in ("argb", "rgb", "hit_id", "hit_t"):
            assert a[plane].dtype == b[plane].dtype and a[plane].dtype.itemsize == 4, (plane, a[plane].dtype)
            # (the float planes as their bits: equal means the same bits, whatever the value)
            assert np.array_equal(a[plane].view(np.uint32), b[plane].view(np.uint32)), (n, budget, wname, plane)
        assert spec_stats[wname] == gen_stats[wname], (n, budget, wname)
        assert gen_stats[wname]["rays_shadow"] > 0 and gen_stats[wname]["pixels_written"] > 0, (wname, gen_stats[wname])


if __name__ == "__main__":
    child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
