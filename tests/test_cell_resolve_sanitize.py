"""The host model of the stage that resolves overflowed per-cell shadow candidate lists, and the packer it reads, under
AddressSanitizer and UndefinedBehaviorSanitizer: tools/cell_resolve_check.cpp, a stand-alone program with its own main, compiled
host-only with csrc/rt_cell_resolve.cpp and the packer, run over semesterbild with text_lowres (every 1000th cell, every list
of it set to the overflow marker).  The walk indexes the threaded tree, the leaf records and the lists by values read from
memory; the sanitizers end the program at the first access outside an array.  No GPU, nothing is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

import scene_update_cases as cases
from test_cell_prune_host import soft_cfg
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, sampling

SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp", "rt_cell_prune.cpp", "rt_cell_resolve.cpp")


def test_host_model_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = tmp_path / "cell_resolve_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                          os.path.join(ROOT, "tools", "cell_resolve_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES] + ["-fsanitize=address,undefined"],
                         capture_output=True, text=True, timeout=600)
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
    run = subprocess.run([str(exe), str(scene), str(_abi.RT_SCENE_BUDGET_DEFAULT), "1000"], capture_output=True, text=True, timeout=600)
    print(run.stdout.strip())
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    got = dict(zip(run.stdout.split()[0::2], (int(v) for v in run.stdout.split()[1::2])))
    assert got["cells"] > 1000 and got["lists_resolved"] > got["left_overflowed"] > 0 and got["emptied"] > 0 and got["slots_listed"] > 0, got
