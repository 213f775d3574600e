"""The host twin of the containment kernel's walk (rt_solid_packed), the closest-point walk before it and the packer they read,
under AddressSanitizer and UndefinedBehaviorSanitizer: tools/solid_check.cpp, a stand-alone program with its own main, compiled
host-only with the packer, run over text_lowres and the icosphere -- as packed and after an LBVH and a PLOC rebuild, and refused
on a split-clipped pack.  The walk indexes the threaded tree, the leaf records and the shading records by values read from
memory and writes rows of R entries per point; the planes hold exactly that many entries, so the sanitizers end the program at
the first access outside an array.  Its totals are the model's.  No GPU, nothing is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

import solid_cases as sc
from test_scene_pack_host import CSRC, HIPCC, ROOT

SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    path = tmp_path_factory.mktemp("solid_check") / "solid_check"
    out = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(path),
                          os.path.join(ROOT, "tools", "solid_check.cpp")] + [os.path.join(CSRC, f) for f in SOURCES] + ["-fsanitize=address,undefined"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return path


@pytest.mark.parametrize("name,r,rule", (("text_lowres", 3, "parity"), ("text_lowres", 8, "winding"), ("ico", 8, "parity"), ("ico", 1, "winding")))
def test_host_twin_runs_clean_under_the_sanitizers(exe, tmp_path, name, r, rule):
    f, p, dirs = sc.scene(name), sc.points(name), sc.table(r)
    n = p.shape[0]
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as fh:
        np.array([f.n_spheres, f.n_triangles, f.materials.shape[0], f.lights.shape[0], n, r], np.uint32).tofile(fh)
        for a, t in ((f.sphere_center, np.float32), (f.sphere_r_sq, np.float32), (f.sphere_r_inv, np.float32), (f.sphere_material, np.uint32),
                     (f.tri_v1, np.float32), (f.tri_e1, np.float32), (f.tri_e2, np.float32), (f.tri_normal, np.float32), (f.tri_material, np.uint32),
                     (f.materials, np.float32), (f.lights, np.float32), (p, np.float32), (dirs, np.float32)):
            np.ascontiguousarray(a, t).tofile(fh)
    want = sc.cached_sd_model(name, r, rule)
    run = subprocess.run([str(exe), str(scene), str(n), str(sc.RULE[rule])], capture_output=True, text=True, timeout=600)
    print(run.stdout.strip())
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    got = dict(zip(run.stdout.split()[0::2], (int(v) for v in run.stdout.split()[1::2])))
    assert got["points"] == n and got["directions"] == r, got
    assert got["inside"] == int(want["inside"].sum()) and got["inside"] > 0, got
    assert got["mixed"] == int(((want["votes"] != 0) & (want["votes"] != r)).sum()), got
    assert got["crossings"] == int(want["crossings"].astype(np.int64).sum()) and got["crossings"] > 0, got
    assert got["winding"] == int(want["winding"].astype(np.int64).sum()), got
    assert got["negative"] == int((want["signed_distance"] < 0).sum()), got
    assert got["slots"] == f.n_triangles and got["same_after_lbvh"] == n and got["same_after_ploc"] == n, got
    assert got["refused"] == (1 if name == "text_lowres" else got["refused"]), got
