"""Radiance queries (rt_trace_rays*) without a GPU: the ABI surface, argument validation, the example program, the
test-side reference checked against the oracle's own render, the camera helpers, and the compiled kernels -- the two new
ones, and every existing one against what it compiled to before the radiance queries existed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes

import kernel_asm
import oracle_lib
import ray_query_cases as rq
import trace_rays_cases as tr

ROOT = rq.ROOT
HEADER = os.path.join(ROOT, "include", "rt_hip.h")
TRACE_FUNCS = ("rt_trace_rays", "rt_trace_rays_device")
RAY_KERNELS = ("rt_rays_kernel", "rt_rays_stream_kernel")


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------
def test_trace_functions_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(rt_[a-z_]+)\s*\(", src, flags=re.M))
    for name in TRACE_FUNCS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    lib = _lib_loaded()
    for name in TRACE_FUNCS:
        assert hasattr(lib, name), name
    assert "#define RT_ABI_VERSION 4u" in open(HEADER).read()


def test_radiance_struct_matches_the_header(tmp_path):
    names = [f for f, _ in _abi.rt_ray_radiance._fields_]
    assert names == ["rgb", "valid", "id", "t", "argb"]
    exprs = ["sizeof(rt_ray_radiance)"] + [f"offsetof(rt_ray_radiance, {f})" for f in names]
    want = [C.sizeof(_abi.rt_ray_radiance)] + [getattr(_abi.rt_ray_radiance, f).offset for f in names]
    prog = tmp_path / "rsz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){\n' +
                    "".join(f'  printf("%zu\\n", (size_t)({e}));\n' for e in exprs) + "  return 0;\n}\n")
    exe = tmp_path / "rsz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_validation_needs_no_device():
    lib = _lib_loaded()
    o = np.zeros((1, 3), np.float32)
    d = np.ones((1, 3), np.float32)
    ids = np.zeros(1, np.int32)
    md = np.ones(1, np.float32)
    cloud = np.zeros((4, 10, 3), np.float32)
    V = _abi.RT_ABI_VERSION

    def params(**kw):
        p, keep = _abi.make_params(RenderConfig.from_features([]))
        for k, v in kw.items():
            if k.startswith("tuning_"):
                setattr(p.tuning, k[7:], v)
            else:
                setattr(p, k, v)
        return p

    good_p = params()
    good_b = _abi.rt_ray_batch(V, 1, o.ctypes.data, d.ctypes.data, None, 0)
    good_r = _abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)
    fake = C.c_void_p(8)  # never dereferenced: every case below fails before the scene is used
    soft = params(light_mult=10, n_cloud_sets=4, cloud_sets=_abi.fptr(cloud))
    cases = [
        ((None, good_p, good_b, good_r), "null scene"),
        ((fake, None, good_b, good_r), "null shading"),
        ((fake, good_p, None, good_r), "null ray batch"),
        ((fake, good_p, good_b, None), "null output"),
        ((fake, params(abi_version=3), good_b, good_r), "rt_params.abi_version"),
        ((fake, good_p, _abi.rt_ray_batch(3, 1, o.ctypes.data, d.ctypes.data, None, 0), good_r), "rt_ray_batch.abi_version"),
        ((fake, good_p, _abi.rt_ray_batch(V, 1, o.ctypes.data, d.ctypes.data, md.ctypes.data, 0), good_r), "max_distance must be NULL"),
        ((fake, good_p, _abi.rt_ray_batch(V, 1, o.ctypes.data, d.ctypes.data, None, _abi.RT_FLAG_BACKFACE_CULLING), good_r), "flags must be 0"),
        ((fake, params(flags=_abi.RT_FLAG_ANTI_ALIASING), good_b, good_r), "RT_FLAG_ANTI_ALIASING"),
        ((fake, good_p, _abi.rt_ray_batch(V, 1, None, d.ctypes.data, None, 0), good_r), "origin / direction"),
        ((fake, good_p, _abi.rt_ray_batch(V, 1, o.ctypes.data, None, None, 0), good_r), "origin / direction"),
        ((fake, good_p, good_b, _abi.rt_ray_radiance()), "every output plane is NULL"),
        # what rt_render rejects in an rt_params
        ((fake, params(light_mult=10), good_b, good_r), "cloud_sets missing"),
        ((fake, params(light_mult=10, n_cloud_sets=0, cloud_sets=_abi.fptr(cloud)), good_b, good_r), "cloud_sets missing"),
        ((fake, params(flags=_abi.RT_FLAG_REFLECTIONS, max_depth_reflection=65), good_b, good_r), "recursion depth"),
        ((fake, params(flags=_abi.RT_FLAG_REFLECTIONS, max_depth_reflection=0, max_depth_refraction=0), good_b, good_r), "depth 0"),
        ((fake, params(flags=_abi.RT_FLAG_REFRACTIONS, max_depth_reflection=0, max_depth_refraction=0), good_b, good_r), "depth 0"),
        ((fake, params(tuning_chunk_log2=5), good_b, good_r), "chunk_log2"),
        ((fake, params(tuning_sort_bits=30), good_b, good_r), "sort_bits"),
        ((fake, params(tuning_shadow_candidate_cap=65), good_b, good_r), "shadow_candidate_cap"),
        ((fake, params(tuning_sub_frames=3), good_b, good_r), "sub_frames"),
        ((fake, params(traversal=7), good_b, good_r), "traversal"),
    ]
    ref = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else C.byref(x))  # noqa: E731
    for args, msg in cases:
        for fn, tail in ((lib.rt_trace_rays, (None,)), (lib.rt_trace_rays_device, (None,))):
            rc = fn(*[ref(a) for a in args], *tail)
            err = lib.rt_last_error().decode()
            # (a depth beyond the library's limit is rt_validate_params' RT_ERR_UNSUPPORTED here as in rt_render)
            assert rc == (_abi.RT_ERR_UNSUPPORTED if msg == "recursion depth" else _abi.RT_ERR_INVALID_ARG), (msg, rc, err)
            assert msg in err, (msg, err)
    # the camera members and the camera's tuning are ignored: nonsense in them is not an error, and neither is n_rays = 0
    # (a no-op that never looks at the scene)
    odd = params(width=0, height=0, win_w=5, win_h=0, n_ranks=3, rank=9, tile_size=1, tuning_levels=99, tuning_phases=99, tuning_tile_order=99)
    empty = _abi.rt_ray_batch(V, 0, None, None, None, 0)
    assert lib.rt_trace_rays(fake, C.byref(odd), C.byref(empty), C.byref(good_r), None) == _abi.RT_OK
    assert lib.rt_trace_rays_device(fake, C.byref(soft), C.byref(empty), C.byref(good_r), None) == _abi.RT_OK


def test_trace_example_links_against_the_abi(tmp_path):
    _lib_loaded()
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_trace_rays_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_trace_rays_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no HIP device" in out.stdout or "with reflections" in out.stdout


# ---- the yardstick: the wrapper equals the oracle's own render, bit for bit, on the camera rays of a full frame ---------------
@pytest.mark.parametrize("features,size", [([], None), (["soft_shadows", "reflections", "refractions"], (96, 80))])
def test_wrapper_equals_the_oracle_render(tmp_path, features, size):
    kw = dict(width_override=size[0], height_override=size[1]) if size else {}
    cfg = RenderConfig.from_features(features, n_cloud_sets=64, **kw)
    assert (cfg.width, cfg.height) == (size or (768, 640))
    flat = scenes.test_scene(cfg).flatten()
    o, d = rq.camera_rays(cfg)  # whole frame: ray index = pixel index
    ref = tr.ref_trace(tr.build_ref(tmp_path), flat, cfg, o, d, argb_fill=0)
    argb, planes, st = oracle_lib.render(flat, cfg)
    hit = planes["hit_id"] >= 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(ref["id"], planes["hit_id"])
    assert np.array_equal(ref["valid"], hit)
    assert np.array_equal(ref["t"][hit].view(np.uint32), planes["hit_t"][hit].view(np.uint32))
    assert np.all(np.isposinf(ref["t"][~hit]))
    assert np.array_equal(ref["rgb"].view(np.uint32), planes["rgb"].view(np.uint32))  # (both 0 on a miss)
    assert np.array_equal(ref["argb"], argb)
    for k in tr.COUNTERS:
        assert ref["counters"][k] == st[k], (k, ref["counters"][k], st[k])
    if features:
        assert st["rays_reflection"] > 0 and st["rays_refraction"] > 0


# ---- camera ------------------------------------------------------------------------------------------------------------
def test_reference_rays_are_the_renders_formula():
    for cfg in (RenderConfig.from_features([]), RenderConfig.from_features(["high_resolution"]),
                RenderConfig.from_features([], width_override=97, height_override=61)):
        o, d = camera.reference_rays(cfg)
        o2, d2 = rq.camera_rays(cfg)
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (cfg.width * cfg.height, 3)
        assert np.array_equal(o.view(np.uint32), o2.view(np.uint32)) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
        # ... and the formula itself, scalar by scalar in float32 (renderer/mod.rs:176-180)
        f = cfg.focus
        for x, y in ((0, 0), (cfg.width - 1, 0), (3, cfg.height - 1), (cfg.width // 2, cfg.height // 3)):
            i = y * cfg.width + x
            ox, oy = np.float32(x) * np.float32(cfg.fw), np.float32(y) * np.float32(cfg.fh)
            assert o[i, 0] == ox and o[i, 1] == oy and o[i, 2] == 0.0
            assert d[i, 0] == ox - np.float32(f.x) and d[i, 1] == oy - np.float32(f.y) and d[i, 2] == np.float32(0.0) - np.float32(f.z)


def test_pinhole_camera():
    eye, target = np.array([-0.7, 0.2, -1.5]), np.array([0.5, 0.4, 0.5])
    for W, H, fov in ((64, 48, 40.0), (33, 57, 75.0)):
        cam = camera.PinholeCamera(eye, target, (0.0, -1.0, 0.0), fov, W, H)
        right, up, fwd = cam.basis()
        B = np.stack([right, up, fwd])
        assert np.allclose(B @ B.T, np.eye(3), atol=1e-12)  # orthonormal
        assert np.allclose(np.cross(fwd, (target - eye)), 0.0, atol=1e-12) and fwd @ (target - eye) > 0
        # the centre ray passes through the target
        c = cam.direction(W / 2.0, H / 2.0)
        s = (target - eye) @ c / (c @ c)
        assert np.allclose(eye + s * c, target, atol=1e-12)
        # the rays through the top and the bottom edge subtend fov_y; pixels are square
        top, bot = cam.direction(W / 2.0, 0.0), cam.direction(W / 2.0, float(H))
        ang = np.degrees(np.arccos(top @ bot / np.linalg.norm(top) / np.linalg.norm(bot)))
        assert abs(ang - fov) < 1e-9
        left, rgt = cam.direction(0.0, H / 2.0), cam.direction(float(W), H / 2.0)
        ang_x = np.arccos(left @ rgt / np.linalg.norm(left) / np.linalg.norm(rgt))
        assert abs(np.tan(ang_x / 2.0) - np.tan(np.radians(fov) / 2.0) * W / H) < 1e-12
        # row-major, row 0 at the top (towards `up`), column 0 at the left
        o, d = cam.rays()
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (W * H, 3)
        assert np.array_equal(o, np.broadcast_to(eye.astype(np.float32), o.shape))
        dd = d.astype(np.float64).reshape(H, W, 3)
        assert np.all(dd[0] @ up > 0) and np.all(dd[-1] @ up < 0)
        assert np.all(dd[:, 0] @ right < 0) and np.all(dd[:, -1] @ right > 0)
        assert np.all(np.diff(dd @ right, axis=1) > 0) and np.all(np.diff(dd @ up, axis=0) < 0)
        assert np.allclose(dd[5, 7], cam.direction(7.5, 5.5), rtol=1e-6)
    with pytest.raises(ValueError):
        camera.PinholeCamera(eye, eye, (0, 1, 0), 40.0, 8, 8).rays()
    with pytest.raises(ValueError):
        camera.PinholeCamera((0, 0, 0), (0, 1, 0), (0, 2, 0), 40.0, 8, 8).rays()


# ---- the compiled kernels ------------------------------------------------------------------------------------------------
# What every kernel compiled to BEFORE the radiance queries: `make asm` (-Rpass-analysis=kernel-resource-usage) at the parent
# commit of the change that added rt_trace_rays ("Pack scenes and frame tables in device-free host code"), hipcc of ROCm as
# installed with this repository's toolchain, gfx950, the Makefile's default flags.
# kernel -> (VGPRs, TotalSGPRs, SGPRs Spill, VGPRs Spill, ScratchSize [bytes/lane], Occupancy [waves/SIMD], LDS Size [bytes/block])
# No margin: the radiance queries add kernels, the existing ones keep their code.
# Three rows moved DOWN since, when the render forms got one copy of their shared rules (profiles/shared_rules.md): SGPR / VGPR
# spills and scratch of rt_classify0_kernel 126 / 34 / 108 -> 124 / 32 / 100, VGPR spills and scratch of rt_primary_pre_kernel
# 22 / 36 -> 20 / 28, SGPR spills of rt_primary_stream_kernel 43 -> 33.  No row may move up.
FIELDS = ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
PINNED = {
    "rt_classify0_kernel": (80, 106, 124, 32, 100, 6, 6304),
    "rt_classify_kernel": (80, 106, 187, 29, 92, 6, 160),
    "rt_compact_kernel": (27, 57, 0, 0, 0, 8, 0),
    "rt_flags_kernel": (77, 94, 0, 0, 0, 6, 0),
    "rt_hard_kernel": (88, 91, 0, 0, 0, 5, 0),
    "rt_hit_kernel": (42, 78, 14, 0, 0, 8, 160),
    "rt_hit_spawn_kernel": (64, 78, 21, 4, 12, 8, 224),
    "rt_primary_kernel": (80, 106, 20, 14, 28, 6, 19616),
    "rt_primary_pre_kernel": (80, 106, 23, 20, 28, 6, 25760),
    "rt_primary_soft10_flags_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_soft10_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_soft19_flags_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_soft19_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_soft28_flags_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_soft28_kernel": (80, 106, 0, 7, 28, 6, 19616),
    "rt_primary_stream_kernel": (80, 104, 33, 20, 32, 6, 25760),
    "rt_query_any_kernel": (55, 89, 0, 0, 0, 8, 0),
    "rt_query_nearest_kernel": (51, 88, 0, 0, 0, 8, 0),
    "rt_resolve_kernel": (20, 26, 0, 0, 0, 8, 0),
    "rt_selftest_math_kernel": (10, 10, 0, 0, 0, 8, 0),
    "rt_sets0_list_kernel": (64, 78, 135, 47, 104, 8, 6304),
    "rt_sets0_walk_kernel": (64, 78, 178, 95, 152, 8, 6304),
    "rt_sets_list_kernel": (64, 78, 25, 35, 64, 8, 160),
    "rt_sets_walk_kernel": (64, 78, 104, 87, 128, 8, 160),
    "rt_shade_kernel": (80, 106, 53, 15, 36, 6, 21664),
    "rt_trace_kernel": (58, 106, 16, 0, 0, 7, 160),
    "rt_trace_spawn_kernel": (65, 106, 58, 0, 0, 7, 224),
}


@pytest.fixture(scope="module")
def compiled():
    """(kernel -> assembly body, kernel -> mangled symbol, kernel -> resource-usage fields) of one `make asm`."""
    c = kernel_asm.compiled("rt_kernels")
    return c.bodies, c.symbols, c.remarks


def test_ray_kernels_are_uniform_walks_at_six_waves(compiled):
    bodies, symbols, remarks = compiled
    for name in RAY_KERNELS:
        assert name in bodies, (name, sorted(bodies))
        assert len(re.findall(r"s_andn2_b64 exec, exec,", bodies[name])) == 0, f"{name}: a divergent loop"
        assert "s_load_dwordx16" in bodies[name], f"{name}: no 64-byte scalar node fetch"
        assert remarks[name]["Occupancy [waves/SIMD]"] == 6, (name, remarks[name])
        # the batch travels as the THIRD kernel argument: process_ray re-reads the first two from fixed kernarg offsets
        assert symbols[name].endswith("E10RtDevScene11RtDevParams9RtRayArgs"), symbols[name]


def test_existing_kernels_compile_to_what_they_did(compiled):
    _, _, remarks = compiled
    assert set(remarks) - set(RAY_KERNELS) == set(PINNED), sorted(set(remarks) ^ set(PINNED) ^ set(RAY_KERNELS))
    for name, want in PINNED.items():
        got = tuple(remarks[name][f] for f in FIELDS)
        assert got == want, (name, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))
