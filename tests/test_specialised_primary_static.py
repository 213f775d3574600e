"""The primary kernels compiled for one configuration (rt_primary_soft*_kernel, CfgSoft in rt_kernels.hip), checked on the
CPU: hipcc cross-compiles gfx950 here.

A specialised kernel exists to carry less than rt_primary_kernel: the same occupancy, no more spilled registers or scratch
than the generic kernel compiled alongside it (compared within one build, not against a literal), wave-uniform loops
only, the scalar 64-byte node fetch.  And the host must send a frame to one only when every constant it was compiled
with holds for that frame (rt_primary_variant, rt_internal.h): the rule is compiled into a small host-only probe here."""
import ctypes as C
import os
import subprocess

import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, scenes

from kernel_asm import CSRC, HIPCC, ROOT, compiled, divergent_loops

GENERIC = "rt_primary_kernel"
SPECIALISED = tuple(f"rt_primary_soft{n}{t}_kernel" for n in (10, 19, 28) for t in ("", "_flags"))


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel)"""
    c = compiled("rt_kernels")
    return c.remarks, c.bodies


def test_every_specialised_kernel_is_built(build):
    remarks, bodies = build
    for name in SPECIALISED + (GENERIC,):
        assert name in remarks and name in bodies, (name, sorted(remarks))


@pytest.mark.parametrize("name", SPECIALISED)
def test_specialised_kernel_keeps_occupancy_and_spills_no_more_than_the_generic(build, name):
    remarks, _ = build
    f, g = remarks[name], remarks[GENERIC]
    print(name, f, "generic:", g)
    assert f["Occupancy [waves/SIMD]"] == 6, (name, f)
    for key in ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]"):
        assert f[key] <= g[key], (name, key, f[key], g[key])


@pytest.mark.parametrize("name", SPECIALISED)
def test_specialised_kernel_has_uniform_loops_and_scalar_node_fetches(build, name):
    _, bodies = build
    n = divergent_loops(bodies[name])
    assert n == 0, f"{name}: {n} divergent loops: some walk or sample loop branches on a per-lane value"
    assert "s_load_dwordx16" in bodies[name], f"{name}: no 64-byte scalar node fetch (a walk lost its uniformity)"


# ---- the selection rule ------------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime.h>
#include "rt_internal.h"
extern "C" const char* pick(int cull, int linear, unsigned n_triangles, unsigned n_spheres, float cloud_delta, unsigned cand_cap,
                            unsigned n_cloud_sets, unsigned light_mult, int flags, int lists, int force_generic) {
  static const uint16_t some_flags[1] = {0};
  static const uint4 some_lists[1] = {};
  RtDevScene sc{};
  RtDevParams p{};
  sc.n_triangles = n_triangles, sc.n_spheres = n_spheres;
  p.flags = RT_FLAG_ANTI_ALIASING | (cull ? RT_FLAG_BACKFACE_CULLING : 0u);
  p.traversal = linear ? RT_TRAVERSAL_LINEAR : RT_TRAVERSAL_BVH;
  p.cloud_delta = cloud_delta, p.cand_cap = cand_cap, p.n_cloud_sets = n_cloud_sets, p.light_mult = light_mult;
  p.recv_flags = flags ? some_flags : nullptr;
  p.cell_lists = lists ? some_lists : nullptr;
  return rt_primary_variant_name(rt_primary_variant(sc, p, force_generic != 0));
}
'''


@pytest.fixture(scope="module")
def pick(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("variant_probe")
    (d / "probe.cpp").write_text(PROBE)
    so = d / "probe.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-shared", "-o", str(so), str(d / "probe.cpp")], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.pick.restype = C.c_char_p
    lib.pick.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_float, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int]

    def call(**kw):
        a = dict(cull=0, linear=0, n_triangles=1000, n_spheres=3, cloud_delta=0.01, cand_cap=64, n_cloud_sets=1024, light_mult=10,
                 flags=1, lists=1, force_generic=0)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.pick(*[a[k] for k in ("cull", "linear", "n_triangles", "n_spheres", "cloud_delta", "cand_cap", "n_cloud_sets",
                                         "light_mult", "flags", "lists", "force_generic")]).decode()

    return call


def config3():
    """What config 3 (bench.py: semesterbild, high_resolution + anti_aliasing + soft_shadows, text.obj) hands the rule."""
    cfg = RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])
    flat = scenes.semesterbild(cfg, "text").flatten()
    return dict(n_triangles=flat.n_triangles, n_spheres=flat.n_spheres, n_cloud_sets=cfg.n_cloud_sets,
                light_mult=cfg.point_light_multiplicator)


def test_config3_selects_its_specialisation_under_both_scene_budgets(pick):
    c3 = config3()
    assert c3["light_mult"] == 10 and c3["n_triangles"] > 0 and c3["n_spheres"] < 32
    assert pick(**c3, flags=1, lists=1) == "rt_primary_soft10_kernel"        # 2 GiB: receiver flags and per-cell lists
    assert pick(**c3, flags=1, lists=0) == "rt_primary_soft10_flags_kernel"  # the default budget: flags only
    assert pick(**c3, flags=1, lists=1, force_generic=1) == GENERIC


def test_every_sample_count_of_the_feature_table_has_both_kernels(pick):
    for n in (10, 19, 28):
        assert pick(light_mult=n, lists=1) == f"rt_primary_soft{n}_kernel"
        assert pick(light_mult=n, lists=0) == f"rt_primary_soft{n}_flags_kernel"


@pytest.mark.parametrize("why, kw", [
    ("backface culling", dict(cull=1)),
    ("linear traversal", dict(linear=1)),
    ("hard shadows", dict(light_mult=1)),
    ("a sample count nothing is compiled for", dict(light_mult=12)),
    ("a cloud table that is not a power of two", dict(n_cloud_sets=1000)),
    ("32 spheres", dict(n_spheres=32)),
    ("more than 32 spheres", dict(n_spheres=40)),
    ("no triangles", dict(n_triangles=0)),
    ("no cloud radius", dict(cloud_delta=0.0)),
    ("candidate sharing off", dict(cand_cap=0)),
    ("no receiver tables", dict(flags=0, lists=0)),
])
def test_anything_else_runs_the_generic_kernel(pick, why, kw):
    for lists in (1, 0):  # under either scene budget
        assert pick(**dict(dict(lists=lists), **kw)) == GENERIC, (why, lists)
