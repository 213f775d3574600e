"""Ray orders (rt_ray_order*, rt_trace_rays_ordered*) without a GPU: the ABI surface, argument validation, the check
behind rt_ray_order_set, the example program, and the HOST MODEL of the order (rt_ray_order_model, csrc/rt_ray_order.cpp).
The model calls the functions of csrc/rt_ray_key.h in loops -- the functions the kernels of rt_order.hip are made of -- so
it is the specification of what a build produces; tests/test_ray_order_gpu.py holds the device to it bit for bit.
Compiled host-only with a probe of its own, the way test_scene_update_host.py probes rt_refit_packed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes

import ray_order_cases as roc
import ray_query_cases as rq

ROOT = rq.ROOT
HEADER = os.path.join(ROOT, "include", "rt_hip.h")
ORDER_FUNCS = ("rt_ray_order_create", "rt_ray_order_destroy", "rt_ray_order_build", "rt_ray_order_build_device", "rt_ray_order_set",
               "rt_ray_order_read", "rt_trace_rays_ordered", "rt_trace_rays_ordered_device")


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------
def test_order_functions_are_declared_and_exported():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(rt_[a-z_]+)\s*\(", src, flags=re.M))
    for name in ORDER_FUNCS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    lib = _lib_loaded()
    for name in ORDER_FUNCS:
        assert hasattr(lib, name), name
    assert "#define RT_ABI_VERSION 4u" in text  # additive: the version stays
    assert "typedef struct rt_ray_order rt_ray_order;" in text  # opaque


def test_order_structs_match_the_header(tmp_path):
    exprs, want = [], []
    for st, names in ((_abi.rt_ray_order_desc, ["abi_version", "capacity", "origin_bits", "reserved"]),
                      (_abi.rt_ray_order_info, ["n_rays", "n_live", "origin_bits", "direction_bits", "n_origin_axes", "n_direction_axes",
                                                "bytes", "device_ms"])):
        assert [f for f, _ in st._fields_] == names
        exprs += [f"sizeof({st.__name__})"] + [f"offsetof({st.__name__}, {f})" for f in names]
        want += [C.sizeof(st)] + [getattr(st, f).offset for f in names]
    prog = tmp_path / "osz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){\n' +
                    "".join(f'  printf("%zu\\n", (size_t)({e}));\n' for e in exprs) + "  return 0;\n}\n")
    exe = tmp_path / "osz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_validation_needs_no_device():
    lib = _lib_loaded()
    V = _abi.RT_ABI_VERSION
    h = C.c_void_p()
    desc = lambda **kw: _abi.rt_ray_order_desc(**{**dict(abi_version=V, capacity=16, origin_bits=0, reserved=0), **kw})  # noqa: E731
    cases = [
        ((None, 0, C.byref(h)), "null argument"),
        ((C.byref(desc()), 0, None), "null argument"),
        ((C.byref(desc(abi_version=3)), 0, C.byref(h)), "abi_version"),
        ((C.byref(desc(capacity=0)), 0, C.byref(h)), "capacity 0"),
        ((C.byref(desc(origin_bits=11)), 0, C.byref(h)), "origin_bits 11"),
        ((C.byref(desc(capacity=(1 << 27) + 1)), 0, C.byref(h)), "capacity"),
        ((C.byref(desc(reserved=1)), 0, C.byref(h)), "reserved"),
    ]
    for args, msg in cases:
        rc = lib.rt_ray_order_create(*args)
        err = lib.rt_last_error().decode()
        assert rc == _abi.RT_ERR_INVALID_ARG and msg in err, (msg, rc, err)
    if lib.rt_device_count() <= 0:
        # valid arguments pass every check and get as far as the device
        assert lib.rt_ray_order_create(C.byref(desc(origin_bits=10)), 0, C.byref(h)) == _abi.RT_ERR_NO_DEVICE
        assert "no HIP device" in lib.rt_last_error().decode() and not h.value
    # NULL handles
    o = np.zeros((1, 3), np.float32)
    d = np.ones((1, 3), np.float32)
    ids = np.zeros(1, np.int32)
    good_b = _abi.rt_ray_batch(V, 1, o.ctypes.data, d.ctypes.data, None, 0)
    good_r = _abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)
    good_p, keep = _abi.make_params(RenderConfig.from_features([]))
    perm = np.zeros(1, np.uint32)
    for rc in (lib.rt_ray_order_build(None, C.byref(good_b)), lib.rt_ray_order_build_device(None, C.byref(good_b), None),
               lib.rt_ray_order_set(None, perm.ctypes.data, 1), lib.rt_ray_order_read(None, None, None, None)):
        assert rc == _abi.RT_ERR_INVALID_ARG and "null ray order" in lib.rt_last_error().decode()
    lib.rt_ray_order_destroy(None)  # a no-op
    # the ordered calls refuse what the plain calls refuse, before the scene or the order is looked at
    fake = C.c_void_p(8)
    assert lib.rt_trace_rays_ordered(None, C.byref(good_p), C.byref(good_b), None, C.byref(good_r), None) == _abi.RT_ERR_INVALID_ARG
    assert "null scene" in lib.rt_last_error().decode()
    assert lib.rt_trace_rays_ordered(fake, C.byref(good_p), None, None, C.byref(good_r), None) == _abi.RT_ERR_INVALID_ARG
    assert "null ray batch" in lib.rt_last_error().decode()
    bad_b = _abi.rt_ray_batch(V, 1, o.ctypes.data, d.ctypes.data, None, _abi.RT_FLAG_BACKFACE_CULLING)
    assert lib.rt_trace_rays_ordered_device(fake, C.byref(good_p), C.byref(bad_b), fake, C.byref(good_r), None) == _abi.RT_ERR_INVALID_ARG
    assert "flags must be 0" in lib.rt_last_error().decode()
    # the device form builds no order of its own
    assert lib.rt_trace_rays_ordered_device(fake, C.byref(good_p), C.byref(good_b), None, C.byref(good_r), None) == _abi.RT_ERR_INVALID_ARG
    assert "null ray order" in lib.rt_last_error().decode()
    # n_rays = 0 without an order: a no-op that never looks at the scene
    empty = _abi.rt_ray_batch(V, 0, None, None, None, 0)
    assert lib.rt_trace_rays_ordered(fake, C.byref(good_p), C.byref(empty), None, C.byref(good_r), None) == _abi.RT_OK


def test_order_example_links_against_the_abi(tmp_path):
    _lib_loaded()
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_ray_order_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_ray_order_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no HIP device" in out.stdout or "same results" in out.stdout


# ---- the device-free source, probed ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return roc.build_probe(tmp_path_factory.mktemp("order_probe"))


def test_permutation_check(probe):
    n = 1000
    rng = np.random.default_rng(1)
    good = rng.permutation(n).astype(np.uint32)
    assert probe.probe_check_permutation(roc.ptr(good), n) == 0
    assert probe.probe_check_permutation(roc.ptr(np.arange(n, dtype=np.uint32)), n) == 0
    dup = good.copy()
    dup[17] = dup[400]
    assert probe.probe_check_permutation(roc.ptr(dup), n) == _abi.RT_ERR_INVALID_ARG
    assert "appears twice" in probe.probe_error().decode()
    far = good.copy()
    far[3] = n
    assert probe.probe_check_permutation(roc.ptr(far), n) == _abi.RT_ERR_INVALID_ARG
    assert "out of range" in probe.probe_error().decode()
    # a short array: the first n - 1 entries of a permutation of [0, n) that still hold ray n - 1
    short = np.ascontiguousarray(np.roll(np.arange(n, dtype=np.uint32), 1)[:n - 1])
    assert (short == n - 1).any()
    assert probe.probe_check_permutation(roc.ptr(short), n - 1) == _abi.RT_ERR_INVALID_ARG
    assert probe.probe_check_permutation(None, 5) == _abi.RT_ERR_INVALID_ARG
    assert probe.probe_check_permutation(None, 0) == 0


def _check_order(keys, perm, n):
    assert keys.shape == perm.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), "not a permutation"
    sk = keys[perm]
    assert np.all(sk[1:] >= sk[:-1]), "keys[perm] decreases"


def test_model_orders_every_kind_of_ray(probe):
    cfg, flat = rq.scene("test_scene")
    o, d = rq.rays(flat, 20000, 21)
    o, d = o.copy(), d.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    dead = np.array([5, 77, 4000, 12345, 19999, 6, 7])
    d[dead[0]] = 0.0
    d[dead[1], 0] = nan
    d[dead[2], 1] = inf
    o[dead[3], 2] = -inf
    o[dead[4], 0] = nan
    d[dead[5]] = 1e-30  # its squared length underflows: the direction normalises to NaN
    o[dead[6], 1] = inf
    keys, perm, info = roc.model(probe, o, d)
    n = o.shape[0]
    _check_order(keys, perm, n)
    assert info["n_rays"] == n and info["n_live"] == n - dead.size
    assert np.all(keys[dead] == 0xFFFFFFFF) and np.all(np.delete(keys, dead) < (1 << 30))
    assert set(perm[-dead.size:].tolist()) == set(dead.tolist()), "dead rays come last"
    assert np.array_equal(perm[-dead.size:], np.sort(dead)), "the model sorts stably"
    # stable everywhere: equal keys keep their batch order
    same = keys[perm][1:] == keys[perm][:-1]
    assert np.all(perm[1:][same] > perm[:-1][same])
    # a shuffled input: the same multiset of (key, original index)
    rng = np.random.default_rng(7)
    sh = rng.permutation(n)
    keys2, perm2, info2 = roc.model(probe, o[sh], d[sh])
    assert info2 == info
    assert np.array_equal(keys2, keys[sh])
    assert sorted(zip(keys2.tolist(), sh.tolist())) == sorted(zip(keys.tolist(), range(n)))


def test_model_edge_cases(probe):
    # identical rays: one key, the identity order
    o = np.tile(np.float32([0.3, 0.2, -1.0]), (300, 1))
    d = np.tile(np.float32([0.1, 0.2, 0.9]), (300, 1))
    keys, perm, info = roc.model(probe, o, d)
    assert np.unique(keys).size == 1 and keys[0] == 0 and np.array_equal(perm, np.arange(300, dtype=np.uint32))
    assert (info["n_origin_axes"], info["n_direction_axes"], info["origin_bits"], info["direction_bits"]) == (0, 0, 0, 0)
    # n = 1, live and dead; n = 0
    keys, perm, info = roc.model(probe, o[:1], d[:1])
    assert keys.tolist() == [0] and perm.tolist() == [0] and info["n_live"] == 1
    keys, perm, info = roc.model(probe, o[:1], np.zeros((1, 3), np.float32))
    assert keys.tolist() == [0xFFFFFFFF] and perm.tolist() == [0] and info["n_live"] == 0
    keys, perm, info = roc.model(probe, o[:0], d[:0])
    assert keys.size == 0 and perm.size == 0 and info["n_rays"] == 0
    # every ray dead
    keys, perm, info = roc.model(probe, o, np.zeros_like(d))
    assert np.all(keys == 0xFFFFFFFF) and np.array_equal(perm, np.arange(300, dtype=np.uint32)) and info["n_live"] == 0
    # origin_bits beyond 10 is refused
    assert roc.model_rc(probe, o, d, origin_bits=11) == _abi.RT_ERR_INVALID_ARG
    # a key's cells: two rays at the two ends of one axis take the first and the last cell
    o2 = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0.25, 0, 0]])
    d2 = np.tile(np.float32([0, 0, 2]), (4, 1))
    keys, perm, info = roc.model(probe, o2, d2)
    assert keys.tolist() == [0, 1023, 512, 256] and perm.tolist() == [0, 3, 2, 1]
    assert (info["n_origin_axes"], info["origin_bits"], info["n_direction_axes"]) == (1, 10, 0)
    # two axes interleave, x the more significant bit of each level
    o3 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    keys, perm, info = roc.model(probe, o3, d2, origin_bits=1)
    assert keys.tolist() == [0, 2, 1, 3] and info["origin_bits"] == 1


def test_model_bit_split(probe):
    cfg = RenderConfig.from_features([], width_override=256, height_override=192)
    o, d = camera.reference_rays(cfg)
    info = roc.model(probe, o, d)[2]
    assert (info["n_origin_axes"], info["origin_bits"], info["n_direction_axes"], info["direction_bits"]) == (2, 10, 3, 3), info
    o, d = roc.pinhole(256, 192).rays()
    info = roc.model(probe, o, d)[2]
    assert (info["n_origin_axes"], info["origin_bits"], info["n_direction_axes"], info["direction_bits"]) == (0, 0, 3, 10), info
    o, d = roc.random_rays(5000, seed=3)
    info = roc.model(probe, o, d)[2]
    # three origin axes and directions: the measured winner, 5 + 5 (profiles/ray_order.md), not all 30 bits to the origins
    assert (info["n_origin_axes"], info["origin_bits"], info["n_direction_axes"], info["direction_bits"]) == (3, 5, 3, 5), info
    # ... unless there is no direction to sort by: parallel rays from a box
    info = roc.model(probe, o, np.tile(np.float32([0, 0, 1]), (o.shape[0], 1)))[2]
    assert (info["n_origin_axes"], info["origin_bits"], info["n_direction_axes"], info["direction_bits"]) == (3, 10, 0, 0), info
    # origin_bits leaves the rest to the directions
    info = roc.model(probe, o, d, origin_bits=10)[2]
    assert (info["origin_bits"], info["direction_bits"]) == (10, 0), info
    info = roc.model(probe, o, d, origin_bits=7)[2]
    assert (info["origin_bits"], info["direction_bits"]) == (7, 3), info


# ---- coherence -------------------------------------------------------------------------------------------------------------
ROW_MAJOR = 65.0  # mean half-perimeter of the pixel bounding boxes of 64 consecutive rays, row-major, 256 pixels wide


def test_the_order_packs_neighbouring_pixels(probe):
    """The condition of the change: the 64-ray runs of the ordered reference-camera batch span at most HALF of what
    row-major runs span (from row-major input and from a shuffle of it), those of a pinhole batch at most two thirds."""
    W, H = 256, 192
    pix = np.arange(W * H)
    assert roc.half_perimeter(pix, W) == ROW_MAJOR
    cfg = RenderConfig.from_features([], width_override=W, height_override=H)
    o, d = camera.reference_rays(cfg)
    perm = roc.model(probe, o, d)[1]
    hp = roc.half_perimeter(pix[perm], W)
    rng = np.random.default_rng(11)
    sh = rng.permutation(W * H)
    perm_sh = roc.model(probe, o[sh], d[sh])[1]
    hp_sh = roc.half_perimeter(sh[perm_sh], W)
    o, d = roc.pinhole(W, H).rays()
    perm_p = roc.model(probe, o, d)[1]
    hp_p = roc.half_perimeter(pix[perm_p], W)
    print(f"mean half-perimeter of 64-ray runs: row-major {ROW_MAJOR}, reference camera ordered {hp:.2f}, from a shuffle {hp_sh:.2f}, "
          f"pinhole ordered {hp_p:.2f}")
    assert hp <= ROW_MAJOR / 2
    assert hp_sh <= ROW_MAJOR / 2
    assert hp_p <= ROW_MAJOR * 2 / 3
