"""The host model of the stage that marks certain glass-pane crossings, under AddressSanitizer and UndefinedBehaviorSanitizer:
tools/cell_through_check.cpp, a stand-alone program with its own main, compiled host-only as tests/test_cell_wide_sanitize.py
compiles its program, run over semesterbild with text_lowres (every 1000th cell and the last one, each with the lists the resolve
stage's walk gives it).  The marks table is allocated exactly as long as its bytes and is written backwards from its end, so a
write before the first cell's bytes or past the last cell's ends the program.  No GPU, nothing is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

import scene_update_cases as cases
from test_cell_prune_host import soft_cfg
from test_cell_resolve_sanitize import SOURCES
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling


def test_host_model_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = tmp_path / "cell_through_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                          os.path.join(ROOT, "tools", "cell_through_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES + ("rt_cell_through.cpp",)] +
                         ["-fsanitize=address,undefined"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    cfg = soft_cfg()
    f = cases.flat_semesterbild(cfg).contiguous()
    cloud = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as fh:
        np.array([f.n_spheres, f.n_triangles, f.materials.shape[0], f.lights.shape[0], cloud.size], np.uint32).tofile(fh)
        for a, t in ((f.sphere_center, np.float32), (f.sphere_r_sq, np.float32), (f.sphere_r_inv, np.float32), (f.sphere_material, np.uint32),
                     (f.tri_v1, np.float32), (f.tri_e1, np.float32), (f.tri_e2, np.float32), (f.tri_normal, np.float32), (f.tri_material, np.uint32),
                     (f.materials, np.float32), (f.lights, np.float32), (cloud, np.float32)):
            np.ascontiguousarray(a, t).tofile(fh)
        np.array([cfg.fw, cfg.fh, cfg.fd, cfg.eps_distance], np.float32).tofile(fh)
    r = subprocess.run([str(exe), str(scene), str(_abi.RT_SCENE_BUDGET_DEFAULT), "1000"], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = dict(zip(r.stdout.split()[0::2], (int(v) for v in r.stdout.split()[1::2])))
    assert got["cells"] > 1000 and got["lists"] > 1000 and got["transmissive"] > 1000, got
    assert 0.3 * got["transmissive"] < got["marked"] <= got["transmissive"], got
