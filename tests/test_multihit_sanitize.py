"""The host twin of the multi-hit kernel's walk (rt_multihit_packed) and the packer it reads, under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/multihit_check.cpp, a stand-alone program with its own main, compiled host-only with the
packer, run over semesterbild with text_lowres -- as packed, with split clipping, and after a rebuild.  The walk indexes the
threaded tree, the leaf records, the material rows and the canonical shading records by values read from memory, and writes
rows of max_hits entries; the planes hold exactly n * max_hits entries, so the sanitizers end the program at the first access
outside an array.  No GPU, nothing is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

import multi_hit_cases as mh
from test_scene_pack_host import CSRC, HIPCC, ROOT

SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")


def test_host_twin_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = tmp_path / "multihit_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                          os.path.join(ROOT, "tools", "multihit_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES] + ["-fsanitize=address,undefined"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    f = mh.scene("text_lowres")
    o, d = mh.rays("text_lowres")
    n = o.shape[0]
    max_d = mh.max_distance("mixed", f, o)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as fh:
        np.array([f.n_spheres, f.n_triangles, f.materials.shape[0], f.lights.shape[0], n], np.uint32).tofile(fh)
        for a, t in ((f.sphere_center, np.float32), (f.sphere_r_sq, np.float32), (f.sphere_r_inv, np.float32), (f.sphere_material, np.uint32),
                     (f.tri_v1, np.float32), (f.tri_e1, np.float32), (f.tri_e2, np.float32), (f.tri_normal, np.float32), (f.tri_material, np.uint32),
                     (f.materials, np.float32), (f.lights, np.float32), (o, np.float32), (d, np.float32), (max_d, np.float32)):
            np.ascontiguousarray(a, t).tofile(fh)
    for k in (5, 16):
        want = mh.model(f, o, d, k)
        for split in (0, 3):
            run = subprocess.run([str(exe), str(scene), str(n), str(split), str(k)], capture_output=True, text=True, timeout=600)
            print(run.stdout.strip())
            assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
            got = dict(zip(run.stdout.split()[0::2], (int(v) for v in run.stdout.split()[1::2])))
            assert got["rays"] == n and got["hits"] == int(want["count"].sum()) and got["objects"] == int(want["total"].sum()), got
            assert got["full"] == int((want["count"] == k).sum()) and got["full"] > 0, got
            assert got["paged"] == int(np.minimum(want["total"] - want["count"], k).sum()), got
            assert got["slots"] >= f.n_triangles and (got["slots"] > f.n_triangles) == (split == 3), got
            assert got["same_after_rebuild"] == (n if split == 0 else 0), got
