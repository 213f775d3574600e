"""The host twin of the ambient-occlusion kernels' walk (rt_occlusion_packed) and the packer it reads, under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/occlusion_check.cpp, a stand-alone program with its own main, compiled host-only with the
packer, run over semesterbild with text_lowres -- as packed, with split clipping, and after an LBVH and a PLOC rebuild.  The
walk indexes the threaded tree, the leaf records, the shading records and the material rows by values read from memory, reads
table rows at (first + s) % n_table and writes (S + 31) / 32 bit words per point; the planes hold exactly that many entries, so
the sanitizers end the program at the first access outside an array.  Its totals are the model's.  No GPU, nothing is loaded
into this process."""
import os
import subprocess

import numpy as np
import pytest

import occlusion_cases as oc
from test_scene_pack_host import CSRC, HIPCC, ROOT

SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")


def test_host_twin_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = tmp_path / "occlusion_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                          os.path.join(ROOT, "tools", "occlusion_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES] + ["-fsanitize=address,undefined"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    name = "text_lowres"
    f = oc.scene(name)
    p, nrm = oc.points(name)
    n, tab, first, bias = p.shape[0], oc.table(), oc.first(p.shape[0]), 1e-4
    max_d = oc.max_distance("fraction", f)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as fh:
        np.array([f.n_spheres, f.n_triangles, f.materials.shape[0], f.lights.shape[0], n, tab.shape[0]], np.uint32).tofile(fh)
        for a, t in ((f.sphere_center, np.float32), (f.sphere_r_sq, np.float32), (f.sphere_r_inv, np.float32), (f.sphere_material, np.uint32),
                     (f.tri_v1, np.float32), (f.tri_e1, np.float32), (f.tri_e2, np.float32), (f.tri_normal, np.float32), (f.tri_material, np.uint32),
                     (f.materials, np.float32), (f.lights, np.float32), (p, np.float32), (nrm, np.float32), (tab, np.float32), (first, np.uint32),
                     (np.array([bias, max_d]), np.float32)):
            np.ascontiguousarray(a, t).tofile(fh)
    for s in (33, 65):  # one sample count of each kernel class, neither a multiple of 32
        free = oc.cached_model(name, s)
        passed = oc.model(f, p, nrm, s, tab, None, bias, np.inf, True)
        limited = oc.cached_model(name, s, kind="fraction")
        for split in (0, 3):
            run = subprocess.run([str(exe), str(scene), str(n), str(split), str(s)], capture_output=True, text=True, timeout=600)
            print(run.stdout.strip())
            assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
            got = dict(zip(run.stdout.split()[0::2], (int(v) for v in run.stdout.split()[1::2])))
            assert got["points"] == n and got["samples"] == s, got
            assert got["clear"] == int(free["clear"].sum()) and got["occluded"] == n * s - got["clear"], got
            assert got["mixed"] == int(((free["clear"] > 0) & (free["clear"] < s)).sum()) and got["mixed"] > 0, got
            assert got["passed"] == int(passed["clear"].sum()) and got["limited"] == int(limited["clear"].sum()), got
            assert got["passed"] > got["clear"] and got["limited"] > got["clear"], got
            assert got["slots"] >= f.n_triangles and (got["slots"] > f.n_triangles) == (split == 3), got
            assert got["same_after_lbvh"] == (n if split == 0 else 0) and got["same_after_ploc"] == (n if split == 0 else 0), got
