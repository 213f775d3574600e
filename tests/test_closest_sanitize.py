"""The host model of the closest-point kernel's walk (rt_closest_packed) and the packer it reads, under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/closest_check.cpp, a stand-alone program with its own main, compiled host-only with the
packer, run over semesterbild with text_lowres -- as packed, with split clipping, and after a rebuild.  The walk indexes the
BVH2, the threaded tree and the leaf records by values read from memory; the sanitizers end the program at the first access
outside an array.  No GPU, nothing is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

import closest_cases as cc
from test_scene_pack_host import CSRC, HIPCC, ROOT

SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")


def test_host_model_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = tmp_path / "closest_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                          os.path.join(ROOT, "tools", "closest_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES] + ["-fsanitize=address,undefined"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    f = cc.scene("text_lowres")
    n = 4000
    pts = cc.points(f, n, seed=51)
    radii = cc.mixed_radii(f, pts, seed=52)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as fh:
        np.array([f.n_spheres, f.n_triangles, f.materials.shape[0], f.lights.shape[0], n], np.uint32).tofile(fh)
        for a, t in ((f.sphere_center, np.float32), (f.sphere_r_sq, np.float32), (f.sphere_r_inv, np.float32), (f.sphere_material, np.uint32),
                     (f.tri_v1, np.float32), (f.tri_e1, np.float32), (f.tri_e2, np.float32), (f.tri_normal, np.float32), (f.tri_material, np.uint32),
                     (f.materials, np.float32), (f.lights, np.float32), (pts, np.float32), (radii, np.float32)):
            np.ascontiguousarray(a, t).tofile(fh)
    want = cc.model(f, pts)
    for split in (0, 3):
        run = subprocess.run([str(exe), str(scene), str(n), str(split)], capture_output=True, text=True, timeout=600)
        print(run.stdout.strip())
        assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
        got = dict(zip(run.stdout.split()[0::2], (int(v) for v in run.stdout.split()[1::2])))
        assert got["points"] == n and got["hits"] == int((want["id"] >= 0).sum()) and got["misses"] == 4, got
        assert got["slots"] >= f.n_triangles and (got["slots"] > f.n_triangles) == (split == 3), got
        assert got["same_after_rebuild"] == (n if split == 0 else 0), got
