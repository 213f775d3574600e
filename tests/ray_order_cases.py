"""Shared pieces of the ray-order tests: the probe over the device-free source (csrc/rt_ray_order.cpp: the host model of
an order and the permutation check), the batches, and the coherence figure."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, camera

from ray_query_cases import ROOT

CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include "rt_ray_key.h"
#include "rt_scene_pack.h"
extern "C" {
int probe_check_permutation(const uint32_t* perm, uint32_t n) { return rt_check_permutation(perm, n); }
int probe_model(const float* o, const float* d, uint32_t n, uint32_t origin_bits, uint32_t* keys, uint32_t* perm, rt_ray_order_info* info) {
  return rt_ray_order_model(o, d, n, origin_bits, keys, perm, info);
}
const char* probe_error() { return rt_last_error(); }
}
'''


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_probe(out_dir) -> C.CDLL:
    """rt_ray_order.cpp (+ rt_scene_pack.cpp and what it links with, for rt_fail), host only: no HIP runtime is touched."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src = os.path.join(str(out_dir), "probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    so = os.path.join(str(out_dir), "probe.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", so, src] +
                   [os.path.join(CSRC, f) for f in ("rt_ray_order.cpp", "rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(so)
    lib.probe_error.restype = C.c_char_p
    lib.probe_check_permutation.argtypes = [C.c_void_p, C.c_uint32]
    lib.probe_model.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(_abi.rt_ray_order_info)]
    return lib


def model_rc(probe, o, d, origin_bits=0):
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    return probe.probe_model(ptr(o), ptr(d), o.shape[0], origin_bits, None, None, None)


def model(probe, o, d, origin_bits=0):
    """-> (keys by ray, permutation, info dict) of the host model."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    keys, perm = np.empty(n, np.uint32), np.empty(n, np.uint32)
    info = _abi.rt_ray_order_info()
    rc = probe.probe_model(ptr(o), ptr(d), n, origin_bits, ptr(keys), ptr(perm), C.byref(info))
    assert rc == 0, probe.probe_error()
    out = info.as_dict()
    del out["bytes"], out["device_ms"]
    return keys, perm, out


def pinhole(width, height):
    """The second viewpoint the coherence figures are stated for."""
    return camera.PinholeCamera((-0.45, 0.25, -1.1), (0.5, 0.5, 0.6), (0.0, -1.0, 0.0), 40.0, width, height)


def random_rays(n, seed):
    """Seeded unrelated rays: origins in the unit box, directions on the sphere."""
    rng = np.random.default_rng(seed)
    o = rng.random((n, 3), np.float32)
    d = rng.standard_normal((n, 3), np.float32)
    return o, d


def half_perimeter(pixels, width):
    """Mean over the runs of 64 consecutive entries of `pixels` (row-major pixel indices) of the half-perimeter of the
    run's pixel bounding box; a last, shorter run counts like the others."""
    pixels = np.asarray(pixels, np.int64)
    x, y = pixels % width, pixels // width
    tot, runs = 0.0, 0
    for a in range(0, pixels.size, 64):
        xs, ys = x[a:a + 64], y[a:a + 64]
        tot += (xs.max() - xs.min() + 1) + (ys.max() - ys.min() + 1)
        runs += 1
    return tot / runs
