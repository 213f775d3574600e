"""Shared pieces of the camera-view tests: frames, sample tables, cameras, and the host models of the ray generator and
the sample resolve (rt_view_rays_model / rt_view_resolve_model, exported by the library; no device needed)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, sampling

# pixel counts that are no multiple of 64 or 256; rows shorter than a wavefront
FRAMES = ((37, 29), (64, 4))
KINDS = {"pinhole": _abi.RT_VIEW_PINHOLE, "reference": _abi.RT_VIEW_REFERENCE}
FILL = 0x00ABCDEF


def sample_tables(kind, cfg=None):
    """name -> (n, 2) float32 offsets for a camera of `kind` (pixels for a pinhole, scene units of `cfg` for the reference's):
    n in {1, 7, 9, 16, 24} -- one packet or fewer, a ragged last packet, more than two packets -- with and without
    bit-identical repeats, one table repeating sample 0."""
    cfg = cfg or RenderConfig.from_features(["anti_aliasing"])
    unit = np.float32([1.0, 1.0]) if kind == _abi.RT_VIEW_PINHOLE else np.float32([cfg.fw, cfg.fh])
    rng = np.random.default_rng(5)
    rnd = lambda n: (rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32) * unit).astype(np.float32)  # noqa: E731
    nine = rnd(9)
    nine[8] = nine[0]  # sample 0 again, in the second packet
    nine[5] = nine[2]
    twenty_four = rnd(24)
    twenty_four[[9, 17, 23]] = twenty_four[[1, 1, 16]]
    twenty_four[12] = twenty_four[0]
    return {
        "centre1": np.zeros((1, 2), np.float32),
        "distinct7": rnd(7),
        "repeats9": nine,
        "config16": camera.view_samples(cfg, kind),  # the reference's deterministic table: 7 of 16 repeat
        "repeats24": twenty_four,
    }


def pinhole(width, height, eye=(0.46, 0.37, -1.9), target=(0.5, 0.45, 0.6), fov=31.0):
    return camera.PinholeCamera(eye=eye, target=target, up=(0.0, -1.0, 0.0), fov_y_deg=fov, width=width, height=height)


def view_camera(kind, cfg, width, height, **pinhole_args):
    return camera.reference_view_camera(cfg) if kind == _abi.RT_VIEW_REFERENCE else pinhole(width, height, **pinhole_args).view_camera()


def frame_config(features, width, height, **kw):
    return RenderConfig.from_features(features, width_override=width, height_override=height, **kw)


def desc(width, height, samples, order=_abi.RT_VIEW_ORDER_ONCE):
    """-> (rt_view_desc, keepalive)"""
    s = np.ascontiguousarray(samples, np.float32)
    return _abi.rt_view_desc(_abi.RT_ABI_VERSION, int(width), int(height), int(s.shape[0]), s.ctypes.data, int(order)), s


def brute_dedup(samples):
    """-> (plane_of, n_distinct) by comparing the offsets as bits, pair by pair"""
    bits = np.ascontiguousarray(samples, np.float32).view(np.uint32)
    firsts, plane_of = [], []
    for k in range(bits.shape[0]):
        same = [u for u, f in enumerate(firsts) if bits[f, 0] == bits[k, 0] and bits[f, 1] == bits[k, 1]]
        if not same:
            firsts.append(k)
        plane_of.append(same[0] if same else len(firsts) - 1)
    return np.array(plane_of, np.uint8), len(firsts)


def model_rays(width, height, samples, cam):
    """rt_view_rays_model -> (origins, directions, plane_of, n_distinct); ray u * width * height + p"""
    d, keep = desc(width, height, samples)
    n = keep.shape[0]
    o, dr = np.empty((n * width * height, 3), np.float32), np.empty((n * width * height, 3), np.float32)
    plane_of, nd = np.empty(n, np.uint8), C.c_uint32()
    _lib.check(_lib.load().rt_view_rays_model(C.byref(d), C.byref(cam), o.ctypes.data, dr.ctypes.data, plane_of.ctypes.data, C.byref(nd)))
    m = nd.value * width * height
    return np.ascontiguousarray(o[:m]), np.ascontiguousarray(dr[:m]), plane_of, nd.value


def resolve_model(n_pixels, n_samples, plane_of, rays, fill=FILL):
    """rt_view_resolve_model on per-ray planes (anything with rgb, valid, id, t: a dict or a Radiance) -> dict of the pixel
    planes rgb, valid, id, t, argb (argb pre-filled with `fill`)."""
    get = (lambda k: rays[k]) if isinstance(rays, dict) else (lambda k: getattr(rays, k))
    rgb, t = np.ascontiguousarray(get("rgb"), np.float32), np.ascontiguousarray(get("t"), np.float32)
    valid, ids = np.ascontiguousarray(get("valid")).astype(np.uint8), np.ascontiguousarray(get("id"), np.int32)
    plane_of = np.ascontiguousarray(plane_of, np.uint8)
    assert rgb.shape == (valid.shape[0], 3) and valid.shape[0] == ids.shape[0] == t.shape[0] == (int(plane_of.max()) + 1) * n_pixels
    out = dict(rgb=np.full((n_pixels, 3), 9.0, np.float32), valid=np.full(n_pixels, 7, np.uint8), id=np.full(n_pixels, -5, np.int32),
               t=np.full(n_pixels, -3.0, np.float32), argb=np.full(n_pixels, fill, np.uint32))
    r = _abi.rt_ray_radiance(rgb.ctypes.data, valid.ctypes.data, ids.ctypes.data, t.ctypes.data, None)
    px = _abi.rt_ray_radiance(*(out[k].ctypes.data for k in ("rgb", "valid", "id", "t", "argb")))
    _lib.check(_lib.load().rt_view_resolve_model(n_pixels, n_samples, plane_of.ctypes.data, C.byref(r), C.byref(px)))
    out["valid"] = out["valid"].astype(bool)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_pixels_equal(got, want, what=""):
    """every pixel plane bit for bit; `got`: a Radiance or a dict, with its argb under got_argb / "argb" when given"""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    for k in ("valid", "id", "t", "rgb"):
        g, w = np.asarray(get(k)), want[k]
        if k == "valid":
            g = g.astype(bool)
        diff = bits(g) != bits(w)
        print(f"{what}: {k} differs in {int(diff.sum())} of {diff.size} words")
        assert not diff.any(), (what, k, np.argwhere(diff)[:5])
