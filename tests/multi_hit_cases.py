"""Shared pieces of the multi-hit tests (host model, host twin and GPU): the test-side reference (tests/multi_hit_ref.c over
oracle/rt_oracle.c, compiled on demand with the oracle's flags), the scenes and rays of tests/ray_query_cases.py, one hand-made
scene with answers known by hand, the kinds of max_distance, and the calls of the model through the library.  Everything is
seeded, so the reference, the model, the kernel's host twin and the device all see the same arrays."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import ray_query_cases as rq
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

F32 = np.float32
SCENES = ("test_scene", "spheres", "triangles", "empty", "text_lowres", "text")
KS = (1, 2, 5, 16)
MAX_D = ("none", "inf", "zero", "negative", "nan", "mixed")
LIST_PLANES = (("id", np.int32, 1), ("t", np.float32, 1), ("point", np.float32, 3), ("normal", np.float32, 3), ("material", np.uint32, 1))
N_RAYS, RAY_SEED = 1021, 7
ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> flat (contiguous FlatScene)"""
    if name == "layers":
        return layers()
    return rq.scene(name)[1].contiguous()


@functools.lru_cache(maxsize=None)
def rays(name):
    """the issue's ray set of a scene: rays(flat, 1021, 7) -- every kind, 100-extent, grazing, on-surface and zero-component ones
    included -- with four dead rays put at the end (zero, NaN and inf directions, a NaN origin)"""
    o, d = rq.rays(scene(name), N_RAYS, RAY_SEED)
    o, d = o.copy(), d.copy()
    d[-1], d[-2], d[-3] = (0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 1.0, 0.0)
    o[-4] = (0.5, np.nan, 0.5)
    return o, d


# ---- the hand-made scene --------------------------------------------------------------------------------------------------
LAYER_Z = [float(z) for z in list(range(1, 11)) + [10] + list(range(12, 41))]  # triangle k lies in z = LAYER_Z[k]; 9 and 10 coincide
LAYER_ORIGIN, LAYER_DIR = (0.25, 0.25, 0.0), (0.0, 0.0, 1.0)


def layers():
    """Sphere 0 (centre = the ray's origin, radius 0.5: the ray starts inside and leaves at t = 0.5), sphere 1 (centre z = 50,
    radius 2: entered at t = 48) and 40 unit triangles (0,0,z) (1,0,z) (0,1,z), z = LAYER_Z: the ray from (0.25, 0.25, 0) along +z
    hits triangle k at t = z exactly (every operation of the literal test is exact for these coordinates)."""
    base = scene("test_scene")
    nt = len(LAYER_Z)
    v1 = np.array([[0.0, 0.0, z] for z in LAYER_Z], F32)
    e1, e2, nrm = np.tile(F32([1, 0, 0]), (nt, 1)), np.tile(F32([0, 1, 0]), (nt, 1)), np.tile(F32([0, 0, 1]), (nt, 1))
    opaque = [i for i in range(base.materials.shape[0]) if base.materials[i][8] == 0.0]  # (column RT_MAT_HAS_OPACITY of rt_hip.h)
    return FlatScene(np.array([LAYER_ORIGIN, (0.25, 0.25, 50.0)], F32), np.array([0.25, 4.0], F32), np.array([2.0, 0.5], F32),
                     np.array([opaque[0], opaque[1 % len(opaque)]], np.uint32), v1, e1, e2, nrm,
                     np.array([opaque[k % len(opaque)] for k in range(nt)], np.uint32), base.materials, base.lights).contiguous()


def layers_answer():
    """-> (ids, ts) of the +z ray in key order: sphere 0, the triangles by z with the coincident pair larger id first, sphere 1"""
    tri = sorted(range(len(LAYER_Z)), key=lambda k: (LAYER_Z[k], -k))
    return [0] + [2 + k for k in tri] + [1], [0.5] + [LAYER_Z[k] for k in tri] + [48.0]


# ---- max_distance ---------------------------------------------------------------------------------------------------------
def max_distance(kind, flat, o, second_t=None, seed=5):
    """none: absent; inf, zero, negative, nan: that value for every ray; mixed: per ray one of +inf, 0, -1, NaN, a length up to
    the scene's extent, or exactly the t of the ray's second hit (`second_t`, where it has one: the test is <=)"""
    n = o.shape[0]
    if kind == "none":
        return None
    if kind != "mixed":
        return np.full(n, {"inf": np.inf, "zero": 0.0, "negative": -1.0, "nan": np.nan}[kind], F32)
    rng = np.random.default_rng(seed)
    lo, hi = rq.bounds(flat)
    ext = float(np.linalg.norm(hi - lo)) or 1.0
    m = (rng.random(n) * ext).astype(F32)
    pick = rng.integers(0, 8, n)
    for k, v in ((0, np.inf), (1, 0.0), (2, -1.0), (3, np.nan)):
        m[pick == k] = v
    if second_t is not None:
        own = (pick == 4) & np.isfinite(second_t)
        m[own] = second_t[own]
    return m


# ---- planes ---------------------------------------------------------------------------------------------------------------
def new_planes(n, k, fill=None):
    out = {name: np.empty((n, k) if cols == 1 else (n, k, cols), dt) for name, dt, cols in LIST_PLANES}
    out["count"], out["total"] = np.empty(n, np.uint32), np.empty(n, np.uint32)
    if fill is not None:
        for a in out.values():
            a.view(np.uint8)[...] = fill
    return out


def lists_struct(out, k, after=None, total=True, only=None):
    h = _abi.rt_ray_hit_lists()
    h.max_hits = k
    if after is not None:
        h.after_t, h.after_id = ptr(after[0]), ptr(after[1])
    for name in out:
        if (name != "total" or total) and (only is None or name in only):
            setattr(h, name, ptr(out[name]))
    return h


def batch_struct(o, d, max_d=None, cull=False):
    b = _abi.rt_ray_batch()
    b.abi_version, b.n_rays = _abi.RT_ABI_VERSION, o.shape[0]
    b.origin, b.direction, b.max_distance = ptr(o), ptr(d), ptr(max_d)
    b.flags = _abi.RT_FLAG_BACKFACE_CULLING if cull else 0
    return b


def model(flat, o, d, k, max_d=None, cull=False, after=None, total=True):
    """rt_list_intersections_model -> dict of planes (`total` None when not asked for)"""
    desc, keep = _abi.make_scene_desc(flat)
    out = new_planes(o.shape[0], k)
    b, h = batch_struct(o, d, max_d, cull), lists_struct(out, k, after, total)
    rc = _lib.load().rt_list_intersections_model(C.byref(desc), C.byref(b), C.byref(h))
    assert rc == 0, _lib.load().rt_last_error()
    if not total:
        out["total"] = None
    return out


def same_bits(got, want):
    """-> names of the planes that differ in some bit (a plane that is None on either side must be None on both)"""
    bad = []
    for name in want:
        a, b = got[name], want[name]
        if a is None or b is None:
            if a is not b:
                bad.append(name)
        elif a.shape != b.shape or not np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)):
            bad.append(name)
    return bad


def chain(call, n, k):
    """Pages through every hit: call(after) -> planes for the cursor `after` ((t, id) arrays or None); each row's last key is fed
    back until no row comes back full.  -> per ray the list of (t bits, id) in the order returned, and the first call's planes."""
    keys = [[] for _ in range(n)]
    after, first = None, None
    for _ in range(10000):
        r = call(after)
        first = first or r
        cnt = r["count"].astype(np.int64)
        for i in np.nonzero(cnt)[0]:
            keys[i] += list(zip(r["t"][i, :cnt[i]].view(np.uint32).tolist(), r["id"][i, :cnt[i]].tolist()))
        full = cnt == k
        if not full.any():
            return keys, first
        # a finished row gets the cursor (+inf, -1), behind which nothing lies: t > inf never, t == inf and id < -1 never
        at = np.where(full, r["t"][:, k - 1], F32(np.inf)).astype(F32)
        ai = np.where(full, r["id"][:, k - 1], -1).astype(np.int32)
        after = (at, ai)
    raise AssertionError("paging did not end")


# ---- the reference ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="multi_hit_ref")
    so = os.path.join(d, "libmulti_hit_ref.so")
    subprocess.check_call(["gcc", *rq.CFLAGS, "-fPIC", "-shared", "-I", os.path.join(rq.ROOT, "include"), "-o", so,
                           os.path.join(rq.HERE, "multi_hit_ref.c"), "-lm", "-lpthread"])
    lib = C.CDLL(so)
    lib.mh_list.restype = None
    lib.mh_list.argtypes = [C.POINTER(_abi.rt_scene_desc), C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 12
    return lib


def ref(flat, o, d, k, max_d=None, cull=False, after=None, total=True):
    """tests/multi_hit_ref.c: the oracle's own tests, a sort, the cursor -> dict of planes"""
    desc, keep = _abi.make_scene_desc(flat)
    out = new_planes(o.shape[0], k)
    at, ai = after if after is not None else (None, None)
    ref_lib().mh_list(C.byref(desc), int(cull), o.shape[0], k, ptr(o), ptr(d), ptr(max_d), ptr(at), ptr(ai), ptr(out["count"]),
                      ptr(out["total"]) if total else None, *[ptr(out[name]) for name, _, _ in LIST_PLANES])
    if not total:
        out["total"] = None
    return out
