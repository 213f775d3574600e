"""Ray queries on the GPU (rt_cast_rays*, rt_any_intersection*) against the oracle-based reference (tests/ray_query_ref.c)
and against the render itself."""
import ctypes as C

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer

import ray_query_cases as rq

pytestmark = pytest.mark.gpu

SCENES = ("test_scene", "text_lowres", "text", "spheres", "triangles", "empty")
_cache = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rq.build_ref(tmp_path_factory.mktemp("rqref"))


def _scene(name):
    if name not in _cache:
        cfg, flat = rq.scene(name)
        _cache[name] = (cfg, flat, DeviceScene(flat, 0))
    return _cache[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_hits_equal(got, want, what):
    for k in ("id", "t", "point", "normal", "material"):
        g, w = _bits(np.asarray(getattr(got, k)).astype(want[k].dtype, copy=False)), _bits(want[k])
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} rays, first {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_nearest_hit_equals_the_oracle(ref, name, cull):
    cfg, flat, ds = _scene(name)
    n = 10000 if name == "text" else 50000
    o, d = rq.rays(flat, n, seed=1 + SCENES.index(name))
    got = ds.cast_rays(o, d, backface_culling=cull)
    want = rq.ref_nearest(ref, flat, o, d, cull)
    _assert_hits_equal(got, want, f"{name} cull={cull}")
    if flat.n_objects:
        assert (want["id"] >= 0).mean() > 0.2, "too few hits to say anything"


def test_camera_rays_equal_the_render():
    cfg = RenderConfig.from_features(["high_resolution", "soft_shadows"])
    _, flat = rq.scene("text")
    r = RaytracerRenderer(cfg, device=0)
    planes = r.render(ImageBuffer.new(cfg.width, cfg.height), flat, aux=True)
    ds = r.device_scene(flat)
    o, d = rq.camera_rays(cfg)
    got = ds.cast_rays(o, d)
    assert np.array_equal(got.id, planes["hit_id"]), np.flatnonzero(got.id != planes["hit_id"])[:10]
    hit = got.id >= 0
    assert hit.mean() > 0.3
    assert np.array_equal(got.t[hit].view(np.uint32), planes["hit_t"][hit].view(np.uint32))


def _segments(flat, ds, n, seed):
    """shadow segments built like the render's (hit points to every light, pushed by eps_distance) + random segments
    with max_distance None-like (+inf), 0, negative, NaN and positive"""
    cfg = RenderConfig.from_features([])
    eps = np.float32(cfg.eps_distance)
    o, d = rq.rays(flat, n, seed)
    h = ds.cast_rays(o, d)
    p = h.point[h.id >= 0]
    L = flat.lights.reshape(-1, 7)[:, :3].astype(np.float32)
    lp = np.repeat(L[None], p.shape[0], axis=0).reshape(-1, 3)
    pp = np.repeat(p, L.shape[0], axis=0)
    ltp = lp - pp
    ld = ltp / np.linalg.norm(ltp, axis=1, keepdims=True).astype(np.float32)
    so = (pp + ld * eps).astype(np.float32)
    md = np.linalg.norm(lp - so, axis=1).astype(np.float32)
    rng = np.random.default_rng(seed)
    ro, rd = rq.rays(flat, n // 2, seed + 100)
    rm = rng.uniform(0.0, 3.0, ro.shape[0]).astype(np.float32)
    k = ro.shape[0] // 8
    rm[:k] = np.inf
    rm[k:2 * k] = 0.0
    rm[2 * k:3 * k] = -rng.uniform(0.0, 1.0, k)
    rm[3 * k:4 * k] = np.nan
    return (np.concatenate([so, ro]).astype(np.float32), np.concatenate([ld, rd]).astype(np.float32),
            np.concatenate([md, rm]).astype(np.float32))


def _assert_occlusion(got, want, what):
    for k in ("has_intersection", "completely_occluded"):
        g = np.asarray(getattr(got, k)).astype(np.uint8)
        bad = np.flatnonzero(g != want[k])
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} rays, first {bad[:5]}"
    dop = np.abs(got.combined_opacity - want["combined_opacity"])
    assert dop.max(initial=0.0) <= 1e-6, f"{what}: opacity off by {dop.max()}"
    clear = want["completely_occluded"] == 0
    df = np.abs(got.color_filter[clear] - want["color_filter"][clear])
    assert df.max(initial=0.0) <= 1e-5, f"{what}: filter off by {df.max()}"


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", ["test_scene", "text_lowres", "spheres"])
def test_occlusion_equals_the_oracle(ref, name, cull):
    cfg, flat, ds = _scene(name)
    o, d, m = _segments(flat, ds, 20000, seed=7)
    got = ds.any_intersection(o, d, m, backface_culling=cull)
    _assert_occlusion(got, rq.ref_any(ref, flat, o, d, m, cull), f"{name} cull={cull}")
    assert got.has_intersection.any() and (~got.has_intersection).any()
    # max_distance NULL = +inf
    got = ds.any_intersection(o, d, None, backface_culling=cull)
    _assert_occlusion(got, rq.ref_any(ref, flat, o, d, None, cull), f"{name} cull={cull} no max_distance")


def test_dead_rays():
    cfg, flat, ds = _scene("test_scene")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    good_o, good_d = np.float32([0.5, 0.4, 0.0]), np.float32([0.0, 0.0, 1.0])
    o = np.array([good_o] * 7, np.float32)
    d = np.array([good_d] * 7, np.float32)
    d[0] = 0.0
    d[1, 0] = nan
    d[2, 1] = inf
    d[3, 2] = -inf
    o[4, 0] = inf
    o[5, 1] = nan
    o[6, 2] = -inf
    h = ds.cast_rays(o, d)
    assert (h.id == -1).all() and np.isposinf(h.t).all()
    assert (h.point == 0).all() and (h.normal == 0).all() and (h.material == 0xFFFFFFFF).all()
    a = ds.any_intersection(o, d)
    assert not a.has_intersection.any() and not a.completely_occluded.any()
    assert (a.combined_opacity == 1.0).all() and (a.color_filter == 1.0).all()
    # NULL planes are not written: only `id` and `combined_opacity` are asked for, the neighbouring memory is a sentinel
    lib = _lib.load()
    ids = np.full(9, 12345, np.int32)
    op = np.full(9, 7.0, np.float32)
    b = _abi.rt_ray_batch(_abi.RT_ABI_VERSION, 7, o.ctypes.data, d.ctypes.data, None, 0)
    _lib.check(lib.rt_cast_rays(ds.handle, C.byref(b), C.byref(_abi.rt_ray_hits(ids[1:].ctypes.data, None, None, None, None))))
    assert ids[0] == 12345 and ids[8] == 12345 and (ids[1:8] == -1).all()
    _lib.check(lib.rt_any_intersection(ds.handle, C.byref(b), C.byref(_abi.rt_ray_occlusion(None, None, op[1:].ctypes.data, None))))
    assert op[0] == 7.0 and op[8] == 7.0 and (op[1:8] == 1.0).all()
    # n_rays = 0 is a no-op
    b.n_rays = 0
    _lib.check(lib.rt_cast_rays(ds.handle, C.byref(b), C.byref(_abi.rt_ray_hits(ids.ctypes.data, None, None, None, None))))


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no
# GPU): the tests that hand tensors to the library run in a child process of their own
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import ctypes as C
import numpy as np
import pytest
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer
import ray_query_cases as rq
import test_ray_query_gpu as T
_scene, _bits = T._scene, T._bits
T.{name}()
print("CHILD-OK")
"""


def _run_child(name):
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here, name=name)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_device_entry_points_with_torch_tensors():
    """The _device entry points on a non-default stream give the bits of the host entry points; bad tensors raise."""
    _run_child("device_entry_points_with_torch_tensors")


def test_query_alongside_a_render_of_the_same_scene():
    _run_child("query_alongside_a_render_of_the_same_scene")


# ---- run in the child process (see CHILD) ---------------------------------------------------------------------------------
def device_entry_points_with_torch_tensors():
    import torch

    cfg, flat, ds = _scene("text_lowres")
    o, d = rq.rays(flat, 30000, seed=5)
    o_m, d_m = rq.rays(flat, 30000, seed=6)
    m = np.random.default_rng(6).uniform(0, 2, o_m.shape[0]).astype(np.float32)
    host_h = ds.cast_rays(o, d, backface_culling=True)
    host_a = ds.any_intersection(o_m, d_m, m)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        th = ds.cast_rays(to, td, backface_culling=True)
        ta = ds.any_intersection(torch.from_numpy(o_m).to(dev), torch.from_numpy(d_m).to(dev), torch.from_numpy(m).to(dev))
    s.synchronize()
    assert isinstance(th.t, torch.Tensor) and th.t.device == dev
    for k in ("id", "t", "point", "normal"):
        assert np.array_equal(_bits(getattr(th, k).cpu().numpy()), _bits(getattr(host_h, k))), k
    assert np.array_equal(th.material.cpu().numpy().view(np.uint32), host_h.material)
    for k in ("has_intersection", "completely_occluded", "combined_opacity", "color_filter"):
        assert np.array_equal(_bits(getattr(ta, k).cpu().numpy()), _bits(getattr(host_a, k))), k
    with pytest.raises(ValueError):
        ds.cast_rays(to.double(), td.double())
    with pytest.raises(ValueError):
        ds.cast_rays(to.cpu(), td.cpu())
    with pytest.raises(ValueError):
        ds.cast_rays(to[:, :2], td[:, :2])


def query_alongside_a_render_of_the_same_scene():
    """A query on one stream while rt_render_device renders the same scene on another, and a host query while a
    progressive render (rt_render_begin) owns the scene: every result equals its solo run."""
    import torch

    cfg = RenderConfig.from_features(["anti_aliasing", "soft_shadows", "reflections", "refractions"])
    _, flat = rq.scene("test_scene")
    r = RaytracerRenderer(cfg, device=0)
    ds = r.device_scene(flat)
    o, d = rq.rays(flat, 200000, seed=9)
    solo_q = ds.cast_rays(o, d)
    lib = _lib.load()
    p, keep = _abi.make_params(cfg)
    dev = torch.device("cuda", 0)
    npx = cfg.width * cfg.height
    s_render, s_query = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    argb_solo = torch.zeros(npx, dtype=torch.int32, device=dev)
    _lib.check(lib.rt_render_device(ds.handle, C.byref(p), argb_solo.data_ptr(), None, C.c_void_p(s_render.cuda_stream)))
    s_render.synchronize()
    argb = torch.zeros(npx, dtype=torch.int32, device=dev)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize()
    _lib.check(lib.rt_render_device(ds.handle, C.byref(p), argb.data_ptr(), None, C.c_void_p(s_render.cuda_stream)))
    with torch.cuda.stream(s_query):
        th = ds.cast_rays(to, td)
    torch.cuda.synchronize()
    assert torch.equal(argb, argb_solo)
    assert np.array_equal(th.id.cpu().numpy(), solo_q.id) and np.array_equal(_bits(th.t.cpu().numpy()), _bits(solo_q.t))
    # progressive render in flight + host query
    buf = np.zeros(npx, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 0, C.byref(h)))
    try:
        q2 = ds.cast_rays(o, d)
    finally:
        st = _abi.rt_stats()
        rc = lib.rt_render_end(h, C.byref(st))
    _lib.check(rc)
    assert np.array_equal(buf.view(np.int32), argb_solo.cpu().numpy())
    assert np.array_equal(q2.id, solo_q.id) and np.array_equal(_bits(q2.t), _bits(solo_q.t))


def test_a_batch_of_2_24_plus_17_rays(ref):
    cfg, flat, ds = _scene("test_scene")
    n = (1 << 24) + 17
    rng = np.random.default_rng(3)
    lo, hi = rq.bounds(flat)
    o = (lo + rng.random((n, 3), np.float32) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((n, 3), np.float32)
    got = ds.cast_rays(o, d)
    sel = np.concatenate([np.arange(0, n, 97), [n - 1]])
    want = rq.ref_nearest(ref, flat, o[sel], d[sel])
    for k in ("id", "t", "point", "normal", "material"):
        assert np.array_equal(_bits(getattr(got, k)[sel]), _bits(want[k])), k
