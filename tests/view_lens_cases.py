"""Shared pieces of the thin-lens view tests: lens tables, the lens struct, wrappers of the host models (rt_view_lens_rays_model /
rt_view_defocus_model, exported by the library; no device needed) and their numpy restatements."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib, camera

import view_cases as vc

INF = float("inf")
F32 = np.float32
# The lenses of the GPU tests.  test_scene's surfaces lie 1.9 to 2.9 units in front of the tests' pinhole camera and the plane at
# 2.5 is in focus.  The test frames are 29 and 4 pixels high where the scene is drawn for 1080, so a pixel is huge and the
# apertures are wide to match: 0.25 units blur the 37 x 29 frame by up to 1.7 pixels, 8 units the 64 x 4 frame by 2 to 5.
# ADAPTIVE: (coc_tol, spread) with which the criterion adds pixels the refine rule left out, and not all of them:
# test_view_lens_host.py::test_the_gpu_lenses_add_some_pixels_and_not_all asserts it on the CPU reference's plane 0.
APERTURE, FOCUS = 0.25, 2.5
APERTURES = {(37, 29): 0.25, (64, 4): 8.0}
ADAPTIVE = {(37, 29): (0.75, 3), (64, 4): (0.5, 3)}


def frame_lens(w, h, adaptive=False, **kw):
    """the GPU tests' lens for a w x h frame; adaptive: with the frame's coc_tol and spread (else the criterion is off)"""
    tol, spread = ADAPTIVE[(w, h)] if adaptive else (INF, 8)
    return lens(**{**dict(aperture=APERTURES[(w, h)], focus_distance=FOCUS, coc_tol=tol, spread=spread), **kw})


def lens(aperture=APERTURE, focus_distance=FOCUS, coc_tol=INF, spread=8, version=_abi.RT_ABI_VERSION, reserved=0):
    return _abi.rt_view_lens(int(version), int(spread), float(aperture), float(focus_distance), float(coc_tol), int(reserved))


def lens_tables():
    """name -> ((n, 2) pixel offsets, (n, 2) lens offsets) for a pinhole camera, n in {1, 7, 9, 16, 24}.  The pixel tables are
    view_cases.sample_tables'; the lens tables repeat and differ so that 4-tuple planes differ from pair planes:
      centre1    one sample through the lens centre
      distinct7  7 distinct pairs, the spiral: 7 planes
      repeats9   pixel offsets 8 == 0 and 5 == 2; lens offset 8 == 0 (sample 0 again, in the second packet: ONE plane) but
                 5 != 2 (same pixel offset, another lens offset: TWO planes) -> 8 planes where the pairs have 7
      config16   the reference's table (9 distinct pairs of 16) with 16 distinct lens offsets: 16 planes
      repeats24  pair repeats 9 == 17 == 1, 23 == 16, 12 == 0; lens repeats 9 == 1, 12 == 0 (one plane each), 17 and 23 differ"""
    px = vc.sample_tables(_abi.RT_VIEW_PINHOLE)
    out = {}
    for name, smp in px.items():
        ls = camera.lens_samples(smp.shape[0]).copy()
        if name == "repeats9":
            ls[8] = ls[0]
        if name == "repeats24":
            ls[9], ls[12] = ls[1], ls[0]
        out[name] = (smp, ls)
    return out


def brute_dedup4(samples, lens_samples):
    """-> (plane_of, n_distinct, first sample of every plane) by comparing the four offsets as bits, sample by sample"""
    bits = np.concatenate([np.ascontiguousarray(samples, F32), np.ascontiguousarray(lens_samples, F32)], axis=1).view(np.uint32)
    firsts, plane_of = [], []
    for k in range(bits.shape[0]):
        same = [u for u, f in enumerate(firsts) if all(bits[f, c] == bits[k, c] for c in range(4))]
        if not same:
            firsts.append(k)
        plane_of.append(same[0] if same else len(firsts) - 1)
    return np.array(plane_of, np.uint8), len(firsts), np.array(firsts)


def model_rays(width, height, samples, lens_samples, cam, ln):
    """rt_view_lens_rays_model -> (origins, directions, plane_of, n_distinct); ray u * width * height + p"""
    d, keep = vc.desc(width, height, samples)
    ls = np.ascontiguousarray(lens_samples, F32)
    n = keep.shape[0]
    o, dr = np.empty((n * width * height, 3), F32), np.empty((n * width * height, 3), F32)
    plane_of, nd = np.empty(n, np.uint8), C.c_uint32()
    _lib.check(_lib.load().rt_view_lens_rays_model(C.byref(d), ls.ctypes.data, C.byref(cam), C.byref(ln), o.ctypes.data, dr.ctypes.data,
                                                   plane_of.ctypes.data, C.byref(nd)))
    m = nd.value * width * height
    return np.ascontiguousarray(o[:m]), np.ascontiguousarray(dr[:m]), plane_of, nd.value


def _ab(width, height, sx, sy, cam):
    """a and b of the pinhole formula for every pixel, float32 operation by operation -> (a, b) of shape (height * width,)"""
    w, h, th = F32(width), F32(height), F32(cam.tan_half_fov_y)
    ys, xs = np.meshgrid(np.arange(height, dtype=F32), np.arange(width, dtype=F32), indexing="ij")
    px = ((xs.ravel() + F32(0.5)).astype(F32) + F32(sx)).astype(F32)
    py = ((ys.ravel() + F32(0.5)).astype(F32) + F32(sy)).astype(F32)
    a = ((((F32(2.0) * px).astype(F32) + -w).astype(F32) / h).astype(F32) * th).astype(F32)
    b = (((h + -(F32(2.0) * py).astype(F32)).astype(F32) / h).astype(F32) * th).astype(F32)
    return a, b


def _d0(a, b, cam, k):
    return ((F32(cam.forward[k]) + (a * F32(cam.right[k])).astype(F32)).astype(F32) + (b * F32(cam.up[k])).astype(F32)).astype(F32)


def numpy_rays(width, height, samples, lens_samples, cam, ln):
    """The lens formula of include/rt_hip.h restated in float32, one rounding per operation, over 4-tuple planes"""
    plane_of, nd, firsts = brute_dedup4(samples, lens_samples)
    n = width * height
    o, d = np.empty((nd * n, 3), F32), np.empty((nd * n, 3), F32)
    A, F = F32(ln.aperture), F32(ln.focus_distance)
    for u, k0 in enumerate(firsts):
        a, b = _ab(width, height, samples[k0][0], samples[k0][1], cam)
        ax, ay = F32(A * F32(lens_samples[k0][0])), F32(A * F32(lens_samples[k0][1]))
        for k in range(3):
            off = F32(F32(ax * F32(cam.right[k])) + F32(ay * F32(cam.up[k])))
            o[u * n:(u + 1) * n, k] = F32(F32(cam.eye[k]) + off)
            d[u * n:(u + 1) * n, k] = ((F * _d0(a, b, cam, k)).astype(F32) + -off).astype(F32)
    return o, d, plane_of, nd


def defocus_model(width, height, sample0, cam, ln, valid0, t0, mask=None):
    """rt_view_defocus_model -> (coc, mask after (bool), n_added)"""
    d, keep = vc.desc(width, height, np.asarray(sample0, F32).reshape(1, 2))
    n = width * height
    v = np.ascontiguousarray(np.asarray(valid0)).astype(np.uint8)
    t = np.ascontiguousarray(t0, F32)
    assert v.shape == (n,) and t.shape == (n,)
    coc = np.full(n, -7.0, F32)
    m = np.zeros(n, np.uint8) if mask is None else np.ascontiguousarray(np.asarray(mask)).astype(np.uint8)
    added = C.c_uint32(12345)
    _lib.check(_lib.load().rt_view_defocus_model(C.byref(d), C.byref(cam), C.byref(ln), v.ctypes.data, t.ctypes.data, coc.ctypes.data, m.ctypes.data,
                                                 C.byref(added)))
    assert set(np.unique(m)) <= {0, 1}
    return coc, m.astype(bool), added.value


def numpy_coc(width, height, sample0, cam, ln, valid0, t0):
    """coc = ((A |z - F|) / (z F)) (H / (2 tan_half)), z = t / |d0|, float32 operation by operation; 0 where invalid"""
    a, b = _ab(width, height, sample0[0], sample0[1], cam)
    dx, dy, dz = (_d0(a, b, cam, k) for k in range(3))
    A, F = F32(ln.aperture), F32(ln.focus_distance)
    with np.errstate(all="ignore"):
        ln2 = (((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32) + (dz * dz).astype(F32)).astype(F32)
        z = (np.asarray(t0, F32) / np.sqrt(ln2).astype(F32)).astype(F32)
        scale = F32(F32(height) / F32(F32(2.0) * F32(cam.tan_half_fov_y)))
        coc = (((A * np.abs((z + -F).astype(F32))).astype(F32) / (z * F).astype(F32)).astype(F32) * scale).astype(F32)
    return np.where(np.asarray(valid0).astype(bool), coc, F32(0.0)).astype(F32)


def brute_spread(width, height, coc, valid0, coc_tol, spread):
    """the criterion as include/rt_hip.h states it, pixel by pixel over the window inside the frame -> picked (bool)"""
    coc = np.asarray(coc, F32).reshape(height, width)
    valid = np.asarray(valid0).astype(bool).reshape(height, width)
    tol = F32(coc_tol)
    out = np.zeros((height, width), bool)
    with np.errstate(invalid="ignore"):
        far = valid & ~(coc <= tol)
        for y in range(height):
            for x in range(width):
                y0, y1, x0, x1 = max(0, y - spread), min(height, y + spread + 1), max(0, x - spread), min(width, x + spread + 1)
                dist = np.maximum(np.abs(np.arange(y0, y1) - y)[:, None], np.abs(np.arange(x0, x1) - x)[None, :]).astype(F32)
                out[y, x] = bool((far[y0:y1, x0:x1] & ~(coc[y0:y1, x0:x1] < dist)).any())
    return out.ravel()
