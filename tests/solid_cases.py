"""Shared pieces of the containment / signed-distance tests (host model, host twin and GPU): the scenes, the point sets, the
direction tables and the calls of the two models through the library.  Everything is seeded, so the references, the model, the
kernel's host twin and the device all see the same arrays.

Scenes: `solids` (Scene API: three slabs, two of them overlapping, and two spheres, one overlapping a slab and holding the other),
`ico` (an icosphere of 1 280 triangles made here, closed, stored normals outward, and one sphere beside it: the smallest input
whose tree has real depth), `text_lowres` (an OPEN mesh), `spheres` and `empty`.

Points of a scene: N_FREE seeded points in the scene's bounds grown by a tenth, N_SURFACE special points, most exactly on
triangles and sphere surfaces (their answers are whatever the model says: they are only compared between the model, the twin and
the device), and N_DEAD dead points at the end (NaN, +inf, -inf coordinates).  501 in all: not a multiple of 64."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import multi_hit_cases as mh
import ray_query_cases as rq
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib, sampling
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Vec3
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import (BoundedPlane, ColorType, FlatScene, Material, PointLight, Scene, SphereData)

F32 = np.float32
SCENES = ("solids", "ico", "text_lowres", "spheres", "empty")
RULES = ("parity", "winding")
RULE = {"parity": _abi.RT_SOLID_RULE_PARITY, "winding": _abi.RT_SOLID_RULE_WINDING}
N_FREE, N_SURFACE, N_DEAD = 486, 12, 3
POINT_SEED = {"solids": 3}  # (test_solid_host.py checks the condition this seed was picked for)
TABLE_SEED = 17
ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

# ---- solids ---------------------------------------------------------------------------------------------------------------------
# slab: (centre, width along x, height along y, depth along z); every number is dyadic, so the known answers are exact
SLABS = (((0.0, 0.0, 0.0), 4.0, 2.0, 1.0), ((1.5, 0.5, 0.25), 2.0, 2.0, 1.0), ((-4.0, 3.0, 1.0), 1.0, 1.0, 2.0))
SOLID_SPHERES = (((0.0, -2.0, 0.0), 1.5), ((0.0, -2.75, 0.0), 0.25))  # the first overlaps slab 0 and holds the second
SLAB_CENTRE = (0.0, 0.0, 0.0)            # of slab 0, outside slab 1 and the spheres: half the smallest side is 0.5
OVERLAP_POINT = (1.25, 0.3125, 0.0625)   # in slabs 0 and 1 (not (1.25, 0.25, 0.125): its ray along (2, -3, 1) leaves slab 1 exactly
                                         # through the diagonal of a face and counts both triangles)
NESTED_POINT = (0.0, -2.75, 0.0)         # the centre of the inner sphere: k_s = 2
FAR_POINT = (40.0, 50.0, 60.0)


def _vec(t):
    return Vec3(F32(t[0]), F32(t[1]), F32(t[2]))


def solids():
    sc = Scene.new()
    colours = (ColorType.new(200, 60, 60), ColorType.new(60, 200, 60), ColorType.new(60, 60, 200))
    for (centre, w, h, d), col in zip(SLABS, colours):
        for t in BoundedPlane.with_material(_vec((0, 0, 1)), _vec(centre), _vec((0, 1, 0)), w, h, d, Material.diffuse(col)).to_basic_geometries():
            sc.add_triangle(t)
    for (centre, r), col in zip(SOLID_SPHERES, colours):
        sc.add_sphere(SphereData.new(_vec(centre), r, col))
    sc.add_light(PointLight.new(_vec((10, 10, 10)), ColorType.new(255, 255, 255), 1.0))
    return sc.flatten().contiguous()


# ---- ico ------------------------------------------------------------------------------------------------------------------------
ICO_CENTRE, ICO_RADIUS, ICO_LEVELS = (0.3, -0.2, 0.5), 1.0, 3  # 20 * 4^3 = 1 280 triangles
ICO_SPHERE = ((3.3, -0.2, 0.5), 0.5)                          # beside it


@functools.lru_cache(maxsize=None)
def ico_mesh():
    """-> (vertices float32 (V, 3), faces int (1280, 3)): the subdivided icosahedron, vertices on the sphere (in float64, cast),
    faces wound so that (v1 - v0) x (v2 - v0) points outward"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(ICO_LEVELS):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    vert = (np.array(ICO_CENTRE) + ICO_RADIUS * np.array(v)).astype(F32)
    return vert, np.array(f, np.int64)


def ico_flat(offset=(0.0, 0.0, 0.0)):
    """the icosphere (moved by `offset`) and ICO_SPHERE as a FlatScene with the materials and lights of test_scene"""
    base = mh.scene("test_scene")
    vert, faces = ico_mesh()
    vert = (vert.astype(np.float64) + np.array(offset, np.float64)).astype(F32)
    v1, v2, v3 = vert[faces[:, 0]], vert[faces[:, 1]], vert[faces[:, 2]]
    e1, e2 = (v2 - v1).astype(F32), (v3 - v1).astype(F32)
    n = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = np.einsum("ij,ij->i", n, v1.astype(np.float64) - (np.array(ICO_CENTRE) + np.array(offset)))
    assert (out > 0).all()
    c, r = ICO_SPHERE
    nt = faces.shape[0]
    return FlatScene(np.array([c], F32), np.array([r * r], F32), np.array([1.0 / r], F32), np.array([0], np.uint32), v1, e1, e2, n.astype(F32),
                     (np.arange(nt) % base.materials.shape[0]).astype(np.uint32), base.materials, base.lights).contiguous()


def ico_inradius():
    """the smallest distance from ICO_CENTRE to a face plane of the float32 mesh, in float64: a ball of this radius lies inside"""
    flat = ico_flat()
    v1, e1, e2 = (a.astype(np.float64) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(np.einsum("ij,ij->i", n, v1 - np.array(ICO_CENTRE)).min())


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "solids":
        return solids()
    if name == "ico":
        return ico_flat()
    return mh.scene(name)


def triangles_only(flat):
    z3, z1, zu = np.zeros((0, 3), F32), np.zeros((0,), F32), np.zeros((0,), np.uint32)
    return FlatScene(z3, z1, z1, zu, flat.tri_v1, flat.tri_e1, flat.tri_e2, flat.tri_normal, flat.tri_material, flat.materials, flat.lights).contiguous()


def extent(flat):
    lo, hi = rq.bounds(flat)
    return float(np.linalg.norm(hi - lo)) or 1.0


# ---- points ---------------------------------------------------------------------------------------------------------------------
FREE, SURFACE, DEAD = slice(0, N_FREE), slice(N_FREE, N_FREE + N_SURFACE), slice(N_FREE + N_SURFACE, None)


def free_points(flat, seed, n=N_FREE):
    lo, hi = rq.bounds(flat)
    grow = 0.1 * (hi - lo)
    rng = np.random.default_rng(seed)
    return ((lo - grow) + rng.random((n, 3)) * (hi - lo + 2 * grow)).astype(F32)


@functools.lru_cache(maxsize=None)
def points(name):
    """-> float32 (501, 3): [FREE] seeded, [SURFACE] exactly on surfaces, [DEAD] dead"""
    flat = scene(name)
    free = free_points(flat, POINT_SEED.get(name, 5))
    surf = []
    if name == "solids":  # the points with answers known by hand are part of the set (the slab's centre is special: see table())
        surf += [np.array(q, F32) for q in (SLAB_CENTRE, OVERLAP_POINT, NESTED_POINT, FAR_POINT)]
    for t in range(min(4, flat.n_triangles)):  # a point of the triangle (of a slab's face: u = v = 1/4 is exact there)
        k = t * max(1, flat.n_triangles // 4)
        surf.append(flat.tri_v1[k] + F32(0.25) * flat.tri_e1[k] + F32(0.25) * flat.tri_e2[k])
    for s in range(min(4, flat.n_spheres)):  # the sphere's +x pole
        surf.append(flat.sphere_center[s] + np.array((np.sqrt(flat.sphere_r_sq[s]), 0, 0), F32))
    surf = np.array(surf, F32).reshape(-1, 3)
    pad = free_points(flat, 99, N_SURFACE - surf.shape[0]) if surf.shape[0] < N_SURFACE else np.zeros((0, 3), F32)
    lo, hi = rq.bounds(flat)
    dead = np.tile((0.5 * (lo + hi)).astype(F32), (N_DEAD, 1))
    dead[0, 0], dead[1, 1], dead[2, 2] = np.nan, np.inf, -np.inf
    p = np.ascontiguousarray(np.concatenate([free, surf[:N_SURFACE], pad, dead]), F32)
    assert p.shape == (N_FREE + N_SURFACE + N_DEAD, 3) and p.shape[0] % 64
    return p


# ---- direction tables -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(r):
    """R = 1: one oblique row; R = 3: sampling.solid_directions(); R = 8: those three, an axis-parallel row (from the centre of a
    slab it leaves exactly through the diagonal of a face: what the default table avoids), a row of length 1e-3 and three seeded
    rows of lengths 0.1 .. 10"""
    if r == 1:
        return np.array([(-0.37, 0.61, 0.7)], F32)
    if r == 3:
        return sampling.solid_directions()
    assert r == 8
    rng = np.random.default_rng(TABLE_SEED)
    u = rq._unit(rng, 4)
    rows = [*sampling.solid_directions(), (0.0, 0.0, 1.0), 1e-3 * u[0], *(u[1:] * 10.0 ** rng.uniform(-1, 1, (3, 1)))]
    return np.ascontiguousarray(np.array(rows), F32)


TABLES = (1, 3, 8)

# ---- calls ------------------------------------------------------------------------------------------------------------------------
SOLID_PLANES = ("inside", "votes", "crossings", "winding")
CLOSEST_PLANES = ("id", "distance", "point", "normal", "bary", "material")
SD_PLANES = ("signed_distance",) + SOLID_PLANES + CLOSEST_PLANES


def new_planes(n, r, names=SD_PLANES, fill=None):
    spec = dict(inside=((n,), np.uint8), votes=((n,), np.uint8), crossings=((n, r), np.uint32), winding=((n, r), np.int32),
                signed_distance=((n,), F32), id=((n,), np.int32), distance=((n,), F32), point=((n, 3), F32), normal=((n, 3), F32),
                bary=((n, 2), F32), material=((n,), np.uint32))
    out = {name: np.empty(*spec[name]) for name in names}
    if fill is not None:
        for a in out.values():
            a.view(np.uint8)[...] = fill
    return out


def batch_struct(p, dirs, rule="parity", max_d=None):
    return _abi.rt_solid_batch(_abi.RT_ABI_VERSION, p.shape[0], ptr(p), ptr(max_d), dirs.shape[0], RULE.get(rule, rule), ptr(dirs))


def solid_struct(out, only=None):
    return _abi.rt_solid_out(*[ptr(out[name]) if name in out and (only is None or name in only) else None for name in SOLID_PLANES])


def sd_struct(out, only=None):
    pick = lambda name: ptr(out[name]) if name in out and (only is None or name in only) else None  # noqa: E731
    return _abi.rt_signed_distance_out(pick("signed_distance"), solid_struct(out, only), _abi.rt_point_hits(*[pick(name) for name in CLOSEST_PLANES]))


def contains_model(flat, p, dirs, rule="parity"):
    """rt_contains_points_model -> dict of planes"""
    desc, keep = _abi.make_scene_desc(flat)
    out = new_planes(p.shape[0], dirs.shape[0], SOLID_PLANES)
    rc = _lib.load().rt_contains_points_model(C.byref(desc), C.byref(batch_struct(p, dirs, rule)), C.byref(solid_struct(out)))
    assert rc == 0, _lib.load().rt_last_error()
    return out


def sd_model(flat, p, dirs, rule="parity", max_d=None):
    """rt_signed_distance_model -> dict of planes"""
    desc, keep = _abi.make_scene_desc(flat)
    out = new_planes(p.shape[0], dirs.shape[0])
    rc = _lib.load().rt_signed_distance_model(C.byref(desc), C.byref(batch_struct(p, dirs, rule, max_d)), C.byref(sd_struct(out)))
    assert rc == 0, _lib.load().rt_last_error()
    return out


def max_distance(flat, n, seed=23):
    """[n] search radii: most a fraction of the extent, some +inf, 0, negative and NaN"""
    rng = np.random.default_rng(seed)
    m = (rng.random(n) * 0.3 * extent(flat)).astype(F32)
    pick = rng.integers(0, 10, n)
    for k, v in ((0, np.inf), (1, 0.0), (2, -1.0), (3, np.nan)):
        m[pick == k] = v
    return m


_MODEL = {}


def cached_sd_model(name, r, rule, with_max_d=False):
    """the signed-distance model's planes on the point set of a scene, computed once per process and left unchanged"""
    key = (name, r, rule, with_max_d)
    if key not in _MODEL:
        flat, p = scene(name), points(name)
        _MODEL[key] = sd_model(flat, p, table(r), rule, max_distance(flat, p.shape[0]) if with_max_d else None)
    return _MODEL[key]


same_bits = mh.same_bits
