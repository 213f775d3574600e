"""Shared pieces of the closest-point tests (host model and GPU): the scenes (tests/ray_query_cases.py's, and one hand-made
scene of degenerate triangles), seeded query points of every kind, the search radii, and the calls of the model through the
library.  Everything is seeded, so the host model, the kernel's host twin and the device all see the same arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene
from ray_query_cases import bounds, scene as ray_scene

F32 = np.float32
SCENES = ("test_scene", "spheres", "triangles", "empty", "degenerate", "text_lowres", "text")
PLANES = (("id", np.int32, 1), ("distance", np.float32, 1), ("point", np.float32, 3), ("normal", np.float32, 3), ("bary", np.float32, 2),
          ("material", np.uint32, 1))

# The float64 bound of tests/test_closest_host.py: tol = K * 2^-23 * max(|p|_inf, largest |coordinate| of the chosen object).
# Largest ratio error / (2^-23 * scale) of rt_closest_points_model against tests/f64_closest.py over exactly the point sets of
# that test (every scene, points(flat, n, seed=11), all three checks, 2000 points each):
#   minimum 0.543 (test_scene), distance 1.751 (text_lowres, text), point 4.137 (degenerate: along the sliver, where the nearest
#   point is ill-conditioned)
# K is 4 times the largest, the margin being for point sets of other seeds.
OBSERVED_RATIO = 4.137
K = 4.0 * OBSERVED_RATIO


# ---- scenes -------------------------------------------------------------------------------------------------------------
# `degenerate`: triangle ids behind the one sphere (id 0)
DEG_PLAIN, DEG_SLIVER, DEG_COLLINEAR, DEG_POINT, DEG_TWIN_A, DEG_TWIN_B, DEG_SHARE_A, DEG_SHARE_B = range(1, 9)


def degenerate():
    """One sphere touching the plain triangle from above, and eight triangles: plain; a sliver of aspect 1e6; collinear
    vertices (zero area: its longest segment is (0,3,0)-(2,3,0), the middle vertex at x = 0.5); three equal vertices; two
    coincident triangles; two triangles sharing the edge (5,0,0)-(5,1,0)."""
    _, base = ray_scene("test_scene")
    v = [((0, 0, 0), (1, 0, 0), (0, 1, 0)),                  # plain, in z = 0
         ((3, 0, 0), (4, 0, 0), (3.5, 1e-6, 0)),             # sliver: base 1, height 1e-6
         ((0, 3, 0), (0.5, 3, 0), (2, 3, 0)),                # collinear
         ((3, 3, 1), (3, 3, 1), (3, 3, 1)),                  # a point
         ((0, 0, 2), (1, 0, 2), (0, 1, 2)),                  # coincident pair
         ((0, 0, 2), (1, 0, 2), (0, 1, 2)),
         ((5, 0, 0), (5, 1, 0), (4, 0.5, 0.5)),              # shared edge x = 5, z = 0
         ((5, 0, 0), (6, 0.5, 0.5), (5, 1, 0))]
    p = np.array(v, np.float64)
    v1, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.maximum(ln, 1e-300), np.array([0.0, 0.0, 1.0]))
    nt = len(v)
    return FlatScene(np.array([[0.25, 0.25, 0.5]], F32), np.array([0.25], F32), np.array([2.0], F32), np.array([1], np.uint32),
                     v1.astype(F32), e1.astype(F32), e2.astype(F32), n.astype(F32), (np.arange(nt) % base.materials.shape[0]).astype(np.uint32),
                     base.materials, base.lights).contiguous()


def scene(name):
    """-> flat (contiguous FlatScene)"""
    if name == "degenerate":
        return degenerate()
    return ray_scene(name)[1].contiguous()


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def points(flat, n, seed):
    """n seeded query points of every kind, float32 (n, 3): in the box; 0.6 to 3 extents outside; 100 extents away; on triangle
    interiors; on shared (or any) edges; exactly at stored vertices (v1, fl(v1 + e1)); 1e-7 .. 1e-3 off a triangle's plane;
    at sphere centres exactly; on and inside spheres; NaN and inf points (two each, wherever n allows)."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(flat)
    ext = float(np.linalg.norm(hi - lo)) or 1.0
    ctr = 0.5 * (lo + hi)
    k = max(n // 10, 1)
    inbox = lambda m: lo + rng.random((m, 3)) * (hi - lo)  # noqa: E731
    P = [inbox(k), ctr + _unit(rng, k) * ext * rng.uniform(0.6, 3.0, (k, 1)), ctr + _unit(rng, k) * ext * 100.0]
    nt = flat.n_triangles
    if nt:
        v1, e1, e2 = (a.astype(np.float64).reshape(-1, 3) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
        ti = rng.integers(0, nt, k)
        u = rng.random((k, 2))
        u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u)
        onface = v1[ti] + e1[ti] * u[:, :1] + e2[ti] * u[:, 1:]
        P.append(onface)
        # on an edge: one of the three, a random position along it (meshes share them)
        ti = rng.integers(0, nt, k)
        t = rng.random((k, 1))
        which = rng.integers(0, 3, k)[:, None]
        a = np.where(which == 2, v1[ti] + e1[ti], v1[ti])
        d = np.where(which == 0, e1[ti], np.where(which == 1, e2[ti], e2[ti] - e1[ti]))
        P.append(a + t * d)
        # stored vertices, as the float32 values the scene holds
        ti = rng.integers(0, nt, k)
        vs = np.where((np.arange(k) % 2 == 0)[:, None], flat.tri_v1[ti], (flat.tri_v1[ti] + flat.tri_e1[ti]).astype(F32))
        P.append(vs.astype(np.float64))
        # just off a plane
        ti = rng.integers(0, nt, k)
        nrm = np.cross(e1[ti], e2[ti])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        u = rng.random((k, 2))
        u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u)
        P.append(v1[ti] + e1[ti] * u[:, :1] + e2[ti] * u[:, 1:] + nrm * 10.0 ** rng.uniform(-7, -3, (k, 1)) * rng.choice([-1, 1], (k, 1)))
    if flat.n_spheres:
        c, r = flat.sphere_center.astype(np.float64), np.sqrt(flat.sphere_r_sq.astype(np.float64))
        si = rng.integers(0, flat.n_spheres, k)
        P.append(flat.sphere_center[si].astype(np.float64))
        P.append(c[si] + _unit(rng, k) * r[si, None] * np.where(np.arange(k) % 2 == 0, 1.0, rng.random(k))[:, None])
    P = np.concatenate(P)
    m = n - P.shape[0]
    if m > 0:
        P = np.concatenate([P, inbox(m)])
    P = np.ascontiguousarray(P[:n], F32)
    if n >= 8:
        P[n - 1], P[n - 2] = (np.nan, 0.5, 0.5), (0.5, 0.5, np.nan)
        P[n - 3], P[n - 4] = (np.inf, 0.5, 0.5), (0.5, -np.inf, 0.5)
    return P


RADII = ("none", "inf", "zero", "negative", "nan", "small", "own")


def radii(flat, pts, kind, own_distance=None):
    """the search radii of `kind` for the points: None, +inf, 0, negative, NaN, 0.05 extents, or the model's own distance (which
    must still count: the test is <=)"""
    n = pts.shape[0]
    lo, hi = bounds(flat)
    ext = float(np.linalg.norm(hi - lo)) or 1.0
    if kind == "none":
        return None
    if kind == "own":
        return np.ascontiguousarray(own_distance, F32)
    value = {"inf": np.inf, "zero": 0.0, "negative": -1.0, "nan": np.nan, "small": 0.05 * ext}[kind]
    return np.full(n, value, F32)


def mixed_radii(flat, pts, seed):
    """one array with every kind of radius in it, seeded"""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(flat)
    ext = float(np.linalg.norm(hi - lo)) or 1.0
    choice = np.array([np.inf, 0.0, -1.0, np.nan, 0.05 * ext, 0.3 * ext, 0.01 * ext], F32)
    return np.ascontiguousarray(choice[rng.integers(0, len(choice), pts.shape[0])], F32)


# ---- the model through the library ------------------------------------------------------------------------------------------
def new_planes(n):
    return {name: np.zeros((n,) if cols == 1 else (n, cols), dt) for name, dt, cols in PLANES}


def batch_struct(pts, max_d):
    return _abi.rt_point_batch(_abi.RT_ABI_VERSION, int(pts.shape[0]), pts.ctypes.data, None if max_d is None else max_d.ctypes.data)


def hits_struct(out):
    return _abi.rt_point_hits(*[out[name].ctypes.data for name, _, _ in PLANES])


def model(flat, pts, max_d=None, bvh=None):
    """rt_closest_points_model: the linear scan.  -> dict of planes"""
    pts = np.ascontiguousarray(pts, F32)
    max_d = None if max_d is None else np.ascontiguousarray(max_d, F32)
    desc, keep = _abi.make_scene_desc(flat, bvh)
    out = new_planes(pts.shape[0])
    b, h = batch_struct(pts, max_d), hits_struct(out)
    _lib.check(_lib.load().rt_closest_points_model(C.byref(desc), C.byref(b), C.byref(h)))
    return out


def same_bits(a, b):
    """every plane equal as bits (a NaN equals itself, -0 differs from +0) -> the names of the planes that differ"""
    bad = []
    for name, _, _ in PLANES:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            bad.append(name)
    return bad
