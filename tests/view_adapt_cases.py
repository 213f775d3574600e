"""Shared pieces of the adaptive-view tests: the refine rule and the stable partition restated in numpy, wrappers of the host
models (rt_view_refine_model / rt_view_resolve_adaptive_model, exported by the library; no device needed), and the
tolerances and cases the CPU and the GPU tests share."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

import view_cases as vc

ID, DEPTH, COLOUR, EVERY = _abi.RT_REFINE_ID, _abi.RT_REFINE_DEPTH, _abi.RT_REFINE_COLOUR, _abi.RT_REFINE_EVERY
# The tolerances of the GPU tests, Python's default criteria (DEPTH | COLOUR).  The test frames are 37 and 64 pixels across a
# scene drawn for 1620: a pixel spans what 25 to 44 pixels of a real frame span, so neighbours differ far more than in a real
# frame and the tolerances are wide to match -- 1/8 of the nearer distance and 1/8 in linear RGB (32 8-bit steps), both exact in
# fp32.  With them the model's mask on the CPU reference's plane-0 trace holds between 5 % and 95 % of the pixels of every
# (shading, view) below: test_view_adaptive_host.py::test_the_gpu_tolerances_refine_some_pixels_and_not_all asserts it.
COLOUR_TOL, DEPTH_TOL = 0.125, 0.125
SOFT = dict(n_cloud_sets=64)
SHADINGS = (([], {}), (["soft_shadows"], SOFT))
# reflections and refractions (a trace with secondary rays blocks and is verified at its end): the two views whose sample 0 sees
# the scene's mirrors and glass in either frame -- the reference camera's top four rows (64 x 4) see none
REALISTIC = (["realistic"], {})
REALISTIC_VIEWS = ("pinhole 37x29 repeats9", "pinhole 64x4 repeats24")
TABLES = ("repeats9", "config16", "repeats24")


def views():
    """(what, width, height, samples, camera) of the adaptive tests: both camera kinds, both frames, the three tables with
    repeats (9 samples / 7 distinct, 16 / 9, 24 / 20)"""
    out = []
    for kind, w, h, table in (("pinhole", 37, 29, "repeats9"), ("reference", 64, 4, "repeats24"), ("pinhole", 37, 29, "config16"),
                              ("reference", 37, 29, "config16"), ("pinhole", 64, 4, "repeats24")):
        cfg = vc.frame_config([], w, h)
        out.append((f"{kind} {w}x{h} {table}", w, h, vc.sample_tables(vc.KINDS[kind], cfg)[table], vc.view_camera(vc.KINDS[kind], cfg, w, h)))
    return out


def scene_flat():
    """test_scene framed for the 37 x 29 reference camera, as tests/test_view_gpu.py frames it"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd import scenes

    return scenes.test_scene(vc.frame_config([], *vc.FRAMES[0])).flatten().contiguous()


def refine(criteria=DEPTH | COLOUR, colour_tol=COLOUR_TOL, depth_tol=DEPTH_TOL):
    return _abi.rt_view_refine(_abi.RT_ABI_VERSION, int(criteria), float(colour_tol), float(depth_tol))


def planes_of(rays, n=None):
    """rgb, valid (uint8), id, t of a dict or a Radiance, contiguous, the first n entries"""
    get = (lambda k: rays[k]) if isinstance(rays, dict) else (lambda k: getattr(rays, k))
    sl = slice(None) if n is None else slice(0, n)
    assert np.asarray(get("rgb")).shape == (np.asarray(get("valid")).shape[0], 3)
    return dict(rgb=np.ascontiguousarray(np.asarray(get("rgb"), np.float32)[sl]), valid=np.ascontiguousarray(np.asarray(get("valid"))[sl]).astype(np.uint8),
                id=np.ascontiguousarray(np.asarray(get("id"), np.int32)[sl]), t=np.ascontiguousarray(np.asarray(get("t"), np.float32)[sl]))


def _radiance(p):
    return _abi.rt_ray_radiance(p["rgb"].ctypes.data, p["valid"].ctypes.data, p["id"].ctypes.data, p["t"].ctypes.data, None)


def refine_model(width, height, rf, plane0):
    """rt_view_refine_model -> (mask as bool, n_refined)"""
    p = planes_of(plane0, width * height)
    mask, n = np.full(width * height, 7, np.uint8), C.c_uint32(12345)
    _lib.check(_lib.load().rt_view_refine_model(width, height, C.byref(rf), C.byref(_radiance(p)), mask.ctypes.data, C.byref(n)))
    assert set(np.unique(mask)) <= {0, 1}
    return mask.astype(bool), n.value


def refine_numpy(width, height, rf, plane0):
    """The refine rule as include/rt_hip.h states it, restated: per pixel, over its up to 8 neighbours inside the frame.  float32 arithmetic, one
    rounding per operation, comparisons negated so that a NaN refines."""
    p = planes_of(plane0, width * height)
    crit, ct, dt = int(rf.criteria), np.float32(rf.colour_tol), np.float32(rf.depth_tol)
    n = width * height
    if crit & EVERY:
        return np.ones(n, bool)
    if not crit & (ID | DEPTH | COLOUR):
        return np.zeros(n, bool)
    valid = p["valid"].reshape(height, width) != 0
    ids, t, rgb = p["id"].reshape(height, width), p["t"].reshape(height, width), p["rgb"].reshape(height, width, 3)
    out = np.zeros((height, width), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                ys, xs = slice(max(0, -dy), height - max(0, dy)), slice(max(0, -dx), width - max(0, dx))    # p
                yq, xq = slice(max(0, dy), height - max(0, -dy)), slice(max(0, dx), width - max(0, -dx))    # q = p + (dx, dy)
                vp, vq = valid[ys, xs], valid[yq, xq]
                r = vp != vq
                if crit & ID:
                    r |= ids[ys, xs] != ids[yq, xq]
                both = vp & vq
                if crit & DEPTH:
                    tp, tq = t[ys, xs], t[yq, xq]
                    diff = np.abs((tp - tq).astype(np.float32))
                    bound = (dt * np.fmin(tp, tq)).astype(np.float32)
                    r |= both & ~(diff <= bound)
                if crit & COLOUR:
                    diff = np.abs((rgb[ys, xs] - rgb[yq, xq]).astype(np.float32))
                    r |= both & (~(diff <= ct)).any(axis=-1)
                out[ys, xs] |= r
    return out.ravel()


def resolve_adaptive_model(n_pixels, n_samples, plane_of, mask, base, rays, fill=vc.FILL):
    """rt_view_resolve_adaptive_model -> dict of the pixel planes (argb pre-filled with `fill`); rays: None or per-ray planes"""
    b = planes_of(base, n_pixels)
    plane_of = np.ascontiguousarray(plane_of, np.uint8)
    m = np.ascontiguousarray(np.asarray(mask)).astype(np.uint8)
    out = dict(rgb=np.full((n_pixels, 3), 9.0, np.float32), valid=np.full(n_pixels, 7, np.uint8), id=np.full(n_pixels, -5, np.int32),
               t=np.full(n_pixels, -3.0, np.float32), argb=np.full(n_pixels, fill, np.uint32))
    px = _abi.rt_ray_radiance(*(out[k].ctypes.data for k in ("rgb", "valid", "id", "t", "argb")))
    r = None
    if rays is not None:
        rp = planes_of(rays)
        assert rp["valid"].shape[0] == (int(plane_of.max()) + 1) * n_pixels
        r = C.byref(_radiance(rp))
    _lib.check(_lib.load().rt_view_resolve_adaptive_model(n_pixels, n_samples, plane_of.ctypes.data, m.ctypes.data, C.byref(_radiance(b)), r, C.byref(px)))
    out["valid"] = out["valid"].astype(bool)
    return out


def where_pixels(mask, full, flat):
    """where(mask, full view's pixel, plane_of == 0 resolve's pixel) for dicts of pixel planes (rgb, valid, id, t, argb)"""
    mask = np.asarray(mask, bool)
    return {k: np.where(mask[:, None] if full[k].ndim == 2 else mask, full[k], flat[k]) for k in full}


def partition_numpy(perm, flags, n_out=None):
    """The stable partition of `perm` (None: the identity) by a flag per ENTRY: set entries first, in their order, then the
    others in theirs; the first n_out entries."""
    flags = np.asarray(flags).astype(bool)
    perm = np.arange(flags.shape[0], dtype=np.uint32) if perm is None else np.asarray(perm, np.uint32)
    out = np.concatenate([perm[flags], perm[~flags]])
    return out if n_out is None else out[:n_out]


def live_flags_numpy(perm, n_pixels, mask):
    """liveness of ray perm[k] = u n_pixels + p in the pass-2 batch: u >= 1 and mask[p]"""
    perm = np.asarray(perm, np.uint32)
    return (perm >= n_pixels) & np.asarray(mask, bool)[perm % n_pixels]
