"""Ray queries (rt_cast_rays*, rt_any_intersection*) without a GPU: the ABI surface, argument validation, the example
program, the compiled kernels, and the test-side reference checked against the float64 model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

import kernel_asm
import ray_query_cases as rq

ROOT = rq.ROOT
HEADER = os.path.join(ROOT, "include", "rt_hip.h")
QUERY_FUNCS = ("rt_cast_rays", "rt_cast_rays_device", "rt_any_intersection", "rt_any_intersection_device")
QUERY_KERNELS = ("rt_query_nearest_kernel", "rt_query_any_kernel")


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_query_functions_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(rt_[a-z_]+)\s*\(", src, flags=re.M))
    for name in QUERY_FUNCS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    lib = _lib_loaded()
    for name in QUERY_FUNCS:
        assert hasattr(lib, name), name


def test_query_structs_match_the_header(tmp_path):
    fields = {"rt_ray_batch": [f for f, _ in _abi.rt_ray_batch._fields_], "rt_ray_hits": [f for f, _ in _abi.rt_ray_hits._fields_],
              "rt_ray_occlusion": [f for f, _ in _abi.rt_ray_occlusion._fields_]}
    exprs = []
    want = []
    for st, names in fields.items():
        exprs.append(f"sizeof({st})")
        want.append(C.sizeof(getattr(_abi, st)))
        for f in names:
            exprs.append(f"offsetof({st}, {f})")
            want.append(getattr(getattr(_abi, st), f).offset)
    prog = tmp_path / "qsz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){\n' +
                    "".join(f'  printf("%zu\\n", (size_t)({e}));\n' for e in exprs) + "  return 0;\n}\n")
    exe = tmp_path / "qsz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


def test_validation_needs_no_device():
    lib = _lib_loaded()
    o = np.zeros((1, 3), np.float32)
    d = np.ones((1, 3), np.float32)
    ids = np.zeros(1, np.int32)
    b = _abi.rt_ray_batch(_abi.RT_ABI_VERSION, 1, o.ctypes.data, d.ctypes.data, None, 0)
    h = _abi.rt_ray_hits(ids.ctypes.data, None, None, None, None)
    occ = _abi.rt_ray_occlusion(ids.ctypes.data, None, None, None)
    fake = C.c_void_p(8)  # never dereferenced: every case below fails before the scene is used
    cases = [
        (lib.rt_cast_rays, (None, C.byref(b), C.byref(h)), "null scene"),
        (lib.rt_cast_rays, (fake, None, C.byref(h)), "null ray batch"),
        (lib.rt_cast_rays, (fake, C.byref(b), None), "null output"),
        (lib.rt_any_intersection, (None, C.byref(b), C.byref(occ)), "null scene"),
        (lib.rt_any_intersection, (fake, None, C.byref(occ)), "null ray batch"),
        (lib.rt_cast_rays_device, (None, C.byref(b), C.byref(h), None), "null scene"),
        (lib.rt_any_intersection_device, (fake, None, C.byref(occ), None), "null ray batch"),
    ]
    for fn, args, msg in cases:
        assert fn(*args) == _abi.RT_ERR_INVALID_ARG
        assert msg in lib.rt_last_error().decode()
    bad = [
        (_abi.rt_ray_batch(3, 1, o.ctypes.data, d.ctypes.data, None, 0), h, "abi_version"),
        (_abi.rt_ray_batch(_abi.RT_ABI_VERSION, 1, o.ctypes.data, d.ctypes.data, None, _abi.RT_FLAG_REFLECTIONS), h, "flag"),
        (_abi.rt_ray_batch(_abi.RT_ABI_VERSION, 1, None, d.ctypes.data, None, 0), h, "origin / direction"),
        (_abi.rt_ray_batch(_abi.RT_ABI_VERSION, 1, o.ctypes.data, None, None, 0), h, "origin / direction"),
        (b, _abi.rt_ray_hits(), "every output plane is NULL"),
    ]
    for bb, hh, msg in bad:
        assert lib.rt_cast_rays(fake, C.byref(bb), C.byref(hh)) == _abi.RT_ERR_INVALID_ARG
        assert msg in lib.rt_last_error().decode(), lib.rt_last_error()
    assert lib.rt_any_intersection(fake, C.byref(b), C.byref(_abi.rt_ray_occlusion())) == _abi.RT_ERR_INVALID_ARG


def test_query_example_links_against_the_abi(tmp_path):
    _lib_loaded()
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_ray_query_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_ray_query_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no HIP device" in out.stdout or "picked object" in out.stdout


def test_query_kernels_compile_without_scratch_and_one_walk_each():
    remarks, bodies, _ = kernel_asm.build("rt_kernels")
    for name in QUERY_KERNELS:
        assert name in bodies, (name, sorted(bodies))
        assert len(re.findall(r"s_andn2_b64 exec, exec,", bodies[name])) <= 1, name
        f = remarks[name]
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (name, f)


def test_reference_agrees_with_the_float64_model(tmp_path):
    """The checker is checked: the oracle-based reference and tests/f64_model.py (independent float64 intersection
    code) name the same nearest object for seeded rays of test_scene, rays the model calls ambiguous excluded."""
    from f64_model import Ambiguous, Model

    lib = rq.build_ref(tmp_path)
    cfg, flat = rq.scene("test_scene")
    o, d = rq.rays(flat, 4000, seed=11)
    # the first six kinds of rq.rays (inside, outside, far, non-unit, zero components, grazing): a ray that STARTS on a
    # surface is decided by the fp32 rounding of its origin, which the float64 model does not always flag as near
    o, d = o[:6 * (4000 // 8)], d[:6 * (4000 // 8)]
    ref = rq.ref_nearest(lib, flat, o, d)
    model = Model(flat, cfg)
    agree = ambiguous = 0
    for i in range(o.shape[0]):
        dd = d[i].astype(np.float64)
        nd = np.linalg.norm(dd)
        try:
            r = model.nearest(o[i].astype(np.float64), dd / nd)
        except Ambiguous:
            ambiguous += 1
            continue
        want = -1 if r is None else r[1]
        assert ref["id"][i] == want, (i, o[i], d[i], ref["id"][i], want)
        agree += 1
    assert agree >= 2500, (agree, ambiguous)
    print(f"reference vs float64 model: {agree} rays agree, {ambiguous} ambiguous (excluded)")
