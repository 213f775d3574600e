"""Shared pieces of the ambient-occlusion tests (host model, host twin and GPU): the point sets, the direction table, the kinds
of max_distance, the calls of the model through the library, and a numpy restatement of the reductions.  Everything is seeded,
so the references, the model, the kernel's host twin and the device all see the same arrays.

Points of a scene (about 500, not a multiple of 64: the last wavefront is partial at every S): the hit points and normals of
rt_list_intersections_model (K = 1) on multi_hit_cases.rays(name), the normal turned towards the ray; seeded free-space points
with random normals of lengths 1e-2 .. 1e2; the normals (0, 0, 1) and (0, 0, -1) -- the latter is the frame's sign switch --
and (0, 0, -0.0 ...) kin; and three dead points at the end: a zero normal, a NaN normal and a non-finite point."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import multi_hit_cases as mh
import ray_query_cases as rq
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

F32 = np.float32
SCENES = ("test_scene", "spheres", "triangles", "empty", "text_lowres")
S_LIST = (1, 2, 7, 32, 33, 64, 65, 129, 256)  # the segment and round boundaries
MAX_D = ("inf", "zero", "negative", "nan", "fraction")
BIASES = (0.0, 1e-4)
N_HITS, N_FREE, N_DEAD = 330, 160, 3
N_TABLE, TABLE_SEED, POINT_SEED = 301, 11, 13
FRACTION = 0.1  # of the scene's extent: the "fraction" kind of max_distance
ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
scene = mh.scene


def extent(flat):
    lo, hi = rq.bounds(flat)
    return float(np.linalg.norm(hi - lo)) or 1.0


def max_distance(kind, flat):
    return {"inf": np.inf, "zero": 0.0, "negative": -1.0, "nan": np.nan, "fraction": FRACTION * extent(flat)}[kind]


@functools.lru_cache(maxsize=None)
def points(name):
    """-> (points, normals) float32 (n, 3); the last N_DEAD are dead"""
    flat = scene(name)
    rng = np.random.default_rng(POINT_SEED)
    o, d = mh.rays(name)
    hit = mh.model(flat, o, d, 1, total=False)
    has = np.flatnonzero(hit["count"] > 0)[:N_HITS]
    p, n = hit["point"][has, 0].copy(), hit["normal"][has, 0].copy()
    away = np.einsum("ij,ij->i", n.astype(np.float64), d[has].astype(np.float64)) > 0
    n[away] = -n[away]
    lo, hi = rq.bounds(flat)
    m = N_FREE + N_HITS - has.size
    free_p = (lo + rng.random((m, 3)) * (hi - lo)).astype(F32)
    free_n = (rq._unit(rng, m) * 10.0 ** rng.uniform(-2, 2, (m, 1))).astype(F32)
    free_n[0], free_n[1], free_n[2], free_n[3] = (0, 0, 1), (0, 0, -1), (0, 0, -3.5), (1e-3, 0, -1)  # around the frame's sign switch
    free_n[4], free_n[5] = (0.0, 1.0, -0.0), (1.0, 0.0, 0.0)  # n.z = -0 and +0: sg follows the sign bit
    ctr = (0.5 * (lo + hi)).astype(F32)
    dead_p = np.tile(ctr, (N_DEAD, 1))
    dead_n = np.array([(0, 0, 0), (np.nan, 1, 0), (0, 1, 0)], F32)
    dead_p[2, 1] = np.inf
    return (np.ascontiguousarray(np.concatenate([p, free_p, dead_p]), F32), np.ascontiguousarray(np.concatenate([n, free_n, dead_n]), F32))


@functools.lru_cache(maxsize=None)
def table():
    """N_TABLE > 256 local directions, cosine-weighted about +z, lengths 0.1 .. 10; row 5 is the zero vector (its ray is dead, so the
    sample counts as occluded), row 6 is +z exactly, row 7 lies in the tangent plane"""
    rng = np.random.default_rng(TABLE_SEED)
    r, phi = np.sqrt(rng.random(N_TABLE)), rng.random(N_TABLE) * 2 * np.pi
    t = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - r * r)], axis=1) * 10.0 ** rng.uniform(-1, 1, (N_TABLE, 1))
    t[5], t[6], t[7] = (0, 0, 0), (0, 0, 1), (1, 0, 0)
    return np.ascontiguousarray(t, F32)


def first(n):
    """[n] start rows: any uint32, so that first + s wraps around the table and around 2^32"""
    rng = np.random.default_rng(TABLE_SEED + 1)
    f = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    edge = np.array((0, N_TABLE - 1, N_TABLE, 0xFFFFFFFF, 0xFFFFFFFF - 100, N_TABLE - 256), np.uint32)[:n]
    f[:edge.size] = edge
    return f


def rows(first_rows, s, n_table):
    """the definition's table rows: ((uint64)first[i] + s) % n_table, (n, S)"""
    f = np.zeros(1, np.uint64) if first_rows is None else first_rows.astype(np.uint64)
    return ((f[:, None] + np.arange(s, dtype=np.uint64)[None, :]) % np.uint64(n_table)).astype(np.int64)


# ---- calls -------------------------------------------------------------------------------------------------------------------
PLANES = ("bits", "clear", "visibility", "bent_normal")


def new_planes(n, s, fill=None):
    out = dict(bits=np.empty((n, (s + 31) // 32), np.uint32), clear=np.empty(n, np.uint32), visibility=np.empty(n, F32), bent_normal=np.empty((n, 3), F32))
    if fill is not None:
        for a in out.values():
            a.view(np.uint8)[...] = fill
    return out


def batch_struct(p, nrm, s, tab, first_rows=None, bias=0.0, max_d=np.inf, flags=0):
    return _abi.rt_occlusion_batch(_abi.RT_ABI_VERSION, p.shape[0], ptr(p), ptr(nrm), s, tab.shape[0], ptr(tab), ptr(first_rows), bias, max_d, flags)


def out_struct(out, only=None):
    return _abi.rt_occlusion_out(*[ptr(out[name]) if only is None or name in only else None for name in PLANES])


def model(flat, p, nrm, s, tab, first_rows=None, bias=0.0, max_d=np.inf, pass_transmissive=False):
    """rt_ambient_occlusion_model -> dict of planes"""
    desc, keep = _abi.make_scene_desc(flat)
    out = new_planes(p.shape[0], s)
    b = batch_struct(p, nrm, s, tab, first_rows, bias, max_d, _abi.RT_OCCLUSION_PASS_TRANSMISSIVE if pass_transmissive else 0)
    rc = _lib.load().rt_ambient_occlusion_model(C.byref(desc), C.byref(b), C.byref(out_struct(out)))
    assert rc == 0, _lib.load().rt_last_error()
    return out


def rays_model(p, nrm, s, tab, first_rows=None, bias=0.0):
    """rt_occlusion_rays_model -> origin (n, 3), direction (n, S, 3) before normalisation, alive (n,) bool"""
    n = p.shape[0]
    o, w, alive = np.empty((n, 3), F32), np.empty((n, s, 3), F32), np.empty(n, np.uint8)
    b = batch_struct(p, nrm, s, tab, first_rows, bias)
    rc = _lib.load().rt_occlusion_rays_model(C.byref(b), ptr(o), ptr(w), ptr(alive))
    assert rc == 0, _lib.load().rt_last_error()
    return o, w, alive.astype(bool)


_MODEL = {}


def cached_model(name, s, first_on=True, bias=1e-4, kind="inf", pass_transmissive=False):
    """the model's planes on the point set, table and start rows of a scene, computed once per process"""
    key = (name, s, first_on, bias, kind, pass_transmissive)
    if key not in _MODEL:
        flat = scene(name)
        p, nrm = points(name)
        _MODEL[key] = model(flat, p, nrm, s, table(), first(p.shape[0]) if first_on else None, bias, max_distance(kind, flat), pass_transmissive)
    return _MODEL[key]


def same_bits(got, want):
    """-> names of the planes that differ in some bit (a plane that is None on either side must be None on both)"""
    return mh.same_bits(got, want)


# ---- the reductions, restated -----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf of float32 arrays: the product is exact in extended precision and the sum rounds once more on the way to float32"""
    L = np.longdouble
    return (np.asarray(a, F32).astype(L) * np.asarray(b, F32).astype(L) + np.asarray(c, F32).astype(L)).astype(F32)


def normalize32(a):
    """rt_mh_normalize: a * (1 / sqrt(fma(a0, a0, fma(a1, a1, a2 * a2)))), one rounding each"""
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        dot = fma32(a[..., 0], a[..., 0], fma32(a[..., 1], a[..., 1], a[..., 2] * a[..., 2]))
        return a * (F32(1) / np.sqrt(dot))[..., None]


def reductions(bits_per_sample, unit, s):
    """occluded (n, S) bool and the unit directions (n, S, 3) -> the planes the definition derives from them"""
    n = bits_per_sample.shape[0]
    occ = bits_per_sample
    words = np.zeros((n, (s + 31) // 32), np.uint32)
    for k in range(s):
        words[:, k // 32] |= occ[:, k].astype(np.uint32) << np.uint32(k % 32)
    clear = (~occ).sum(axis=1).astype(np.uint32)
    with np.errstate(all="ignore"):
        q = np.where(occ[..., None], 0, np.rint(unit * F32(1048576.0))).astype(np.int64)
        total = q.sum(axis=1)
        assert np.abs(total).max(initial=0) < 2 ** 31
        bent = normalize32(total.astype(F32))
    bent[(total == 0).all(axis=1)] = 0
    return dict(bits=words, clear=clear, visibility=(clear.astype(F32) / F32(s)).astype(F32), bent_normal=bent.astype(F32))


def unpack(bits, s):
    """bit words (n, W) -> occluded (n, S) bool; asserts that the unused high bits are 0"""
    k = np.arange(s)
    occ = ((bits[:, k // 32] >> (k % 32).astype(np.uint32)) & 1).astype(bool)
    if s % 32:
        assert (bits[:, -1] >> np.uint32(s % 32) == 0).all()
    return occ
