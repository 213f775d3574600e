"""Shared pieces of the ray-query tests: the test-side reference (tests/ray_query_ref.c over oracle/rt_oracle.c, compiled
on demand with the oracle's flags), the scenes and the seeded ray kinds."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# oracle/Makefile's flags
CFLAGS = ["-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-pthread"]


def build_ref(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "libray_query_ref.so")
    subprocess.check_call(["gcc", *CFLAGS, "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "ray_query_ref.c"), "-lm", "-lpthread"])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.rq_nearest.restype = None
    lib.rq_nearest.argtypes = [C.POINTER(_abi.rt_scene_desc), C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    lib.rq_any.restype = None
    lib.rq_any.argtypes = [C.POINTER(_abi.rt_scene_desc), C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    return lib


def ref_nearest(lib, flat, o, d, cull=False):
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    desc, keep = _abi.make_scene_desc(flat)
    out = dict(id=np.empty(n, np.int32), t=np.empty(n, np.float32), point=np.empty((n, 3), np.float32),
               normal=np.empty((n, 3), np.float32), material=np.empty(n, np.uint32))
    lib.rq_nearest(C.byref(desc), int(cull), n, o.ctypes.data, d.ctypes.data, out["id"].ctypes.data, out["t"].ctypes.data,
                   out["point"].ctypes.data, out["normal"].ctypes.data, out["material"].ctypes.data)
    return out


def ref_any(lib, flat, o, d, max_d=None, cull=False):
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    desc, keep = _abi.make_scene_desc(flat)
    m = None if max_d is None else np.ascontiguousarray(max_d, np.float32)
    out = dict(has_intersection=np.empty(n, np.uint8), completely_occluded=np.empty(n, np.uint8),
               combined_opacity=np.empty(n, np.float32), color_filter=np.empty((n, 3), np.float32))
    lib.rq_any(C.byref(desc), int(cull), n, o.ctypes.data, d.ctypes.data, None if m is None else m.ctypes.data,
               out["has_intersection"].ctypes.data, out["completely_occluded"].ctypes.data, out["combined_opacity"].ctypes.data,
               out["color_filter"].ctypes.data)
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def c3_config():
    return RenderConfig.from_features(["high_resolution", "anti_aliasing", "soft_shadows"])


def scene(name):
    """-> (cfg, flat).  test_scene, spheres, triangles, empty, text_lowres, text (semesterbild)."""
    if name in ("text", "text_lowres"):
        cfg = c3_config()
        return cfg, scenes.semesterbild(cfg, name).flatten()
    cfg = RenderConfig.from_features([])
    flat = scenes.test_scene(cfg).flatten()
    z3, z1, zu = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32), np.zeros((0,), np.uint32)
    if name == "spheres":
        flat = flat.without_triangles()
    elif name == "triangles":
        flat = FlatScene(z3, z1, z1, zu, flat.tri_v1, flat.tri_e1, flat.tri_e2, flat.tri_normal, flat.tri_material,
                         flat.materials, flat.lights)
    elif name == "empty":
        flat = FlatScene(z3, z1, z1, zu, z3, z3, z3, z3, zu, flat.materials, flat.lights)
    return cfg, flat


def bounds(flat):
    pts = [flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None], flat.sphere_center + np.sqrt(flat.sphere_r_sq)[:, None],
           flat.tri_v1, flat.tri_v1 + flat.tri_e1, flat.tri_v1 + flat.tri_e2]
    pts = [p.reshape(-1, 3) for p in pts if p.size]
    if not pts:
        return np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    allp = np.concatenate(pts).astype(np.float64)
    return allp.min(axis=0), allp.max(axis=0)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rays(flat, n, seed):
    """n seeded rays of every kind: origins inside, outside and 100x the extent away; unit and non-unit directions;
    directions with zero components; rays that graze a triangle's plane; rays that start on a surface.  -> (o, d) float32."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(flat)
    ext = float(np.linalg.norm(hi - lo)) or 1.0
    ctr = 0.5 * (lo + hi)
    k = n // 8
    inbox = lambda m: lo + rng.random((m, 3)) * (hi - lo)  # noqa: E731
    O, D = [], []
    # inside, random directions
    O.append(inbox(k)), D.append(_unit(rng, k))
    # outside (0.6 .. 3 extents away), aimed at points of the box
    o = ctr + _unit(rng, k) * ext * rng.uniform(0.6, 3.0, (k, 1))
    O.append(o), D.append(inbox(k) - o)
    # 100x the extent away, aimed at the box
    o = ctr + _unit(rng, k) * ext * 100.0
    O.append(o), D.append(inbox(k) - o)
    # non-unit directions (lengths 1e-2 .. 1e2)
    O.append(inbox(k)), D.append(_unit(rng, k) * 10.0 ** rng.uniform(-2, 2, (k, 1)))
    # zero components: one or two axes zeroed
    o = inbox(k)
    d = _unit(rng, k)
    for j in range(k):
        ax = rng.choice(3, size=1 + (j % 2), replace=False)
        d[j, ax] = 0.0
        if not d[j].any():
            d[j, (ax[0] + 1) % 3] = 1.0
    O.append(o), D.append(d)
    nt = flat.n_triangles
    if nt:
        v1, e1, e2 = (a.astype(np.float64).reshape(-1, 3) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
        # graze a triangle's plane: start in the plane (1e-7 .. 1e-3 off it), aim at its centroid within the plane
        ti = rng.integers(0, nt, k)
        nrm = np.cross(e1[ti], e2[ti])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        cen = v1[ti] + (e1[ti] + e2[ti]) / 3.0
        inplane = np.cross(nrm, _unit(rng, k))
        o = cen + inplane * ext * rng.uniform(0.05, 0.5, (k, 1)) + nrm * 10.0 ** rng.uniform(-7, -3, (k, 1)) * rng.choice([-1, 1], (k, 1))
        O.append(o), D.append(cen - o)
        # start on a triangle
        ti = rng.integers(0, nt, k)
        u = rng.random((k, 2))
        u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u)
        o = v1[ti] + e1[ti] * u[:, :1] + e2[ti] * u[:, 1:]
        O.append(o), D.append(_unit(rng, k))
    if flat.n_spheres:
        # start on a sphere
        si = rng.integers(0, flat.n_spheres, k)
        o = flat.sphere_center.astype(np.float64)[si] + _unit(rng, k) * np.sqrt(flat.sphere_r_sq.astype(np.float64))[si, None]
        O.append(o), D.append(_unit(rng, k))
    O, D = np.concatenate(O), np.concatenate(D)
    m = n - O.shape[0]
    if m > 0:
        O, D = np.concatenate([O, inbox(m)]), np.concatenate([D, _unit(rng, m)])
    return np.ascontiguousarray(O[:n], np.float32), np.ascontiguousarray(D[:n], np.float32)


def camera_rays(cfg):
    """The camera rays of a frame without anti-aliasing: origin (x fw, y fh, 0), direction origin - focus (the
    render's primary ray, raytracer_renderer.rs:1190-1357), row-major."""
    W, H = cfg.width, cfg.height
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    o = np.zeros((H * W, 3), np.float32)
    o[:, 0] = xs.ravel() * np.float32(cfg.fw)
    o[:, 1] = ys.ravel() * np.float32(cfg.fh)
    f = cfg.focus
    d = o - np.array([f.x, f.y, f.z], np.float32)
    return o, np.ascontiguousarray(d, np.float32)
