"""Radiance queries on the GPU (rt_trace_rays*): the render's camera rays as a batch against the render itself (bit for
bit), arbitrary rays against the oracle-based reference (tests/trace_rays_ref.c, the bars of tests/test_parity_gpu.py),
and what is particular to batches -- every batch with secondary rays is verified, and the render state survives them."""
import ctypes as C

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import F, Vec3
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import (BoundedPlane, ColorType, Material, PointLight, Scene, SphereData,
                                                            TransmissionProperties)

import ray_query_cases as rq
import trace_rays_cases as tr

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("trref"))


def _scene(name):
    if name not in _cache:
        cfg, flat = rq.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- camera rays equal the render ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,features", [
    ("test_scene", []),
    ("test_scene", ["realistic", "soft_shadows"]),
    ("text", ["high_resolution", "soft_shadows"]),
    ("text", ["high_resolution", "realistic", "soft_shadows"]),
])
def test_camera_rays_equal_the_render(scene, features):
    """trace_rays(reference_rays(cfg)) is the frame without anti-aliasing: same process_ray, sums through the same
    order-independent fixed-point accumulator -- id equal, t and rgb bit-equal on hits, argb equal with misses untouched."""
    cfg = RenderConfig.from_features(features)
    flat = scenes.test_scene(cfg).flatten() if scene == "test_scene" else scenes.semesterbild(cfg, "text").flatten()
    r = RaytracerRenderer(cfg, device=0)
    fill = 0x00123456
    buf = ImageBuffer.new_with_color(cfg.width, cfg.height, fill)
    planes = r.render(buf, flat, aux=True)
    frame_stats = r.last_stats
    ds = r.device_scene(flat)
    o, d = camera.reference_rays(cfg)
    argb = np.full(o.shape[0], fill, np.uint32)
    got = ds.trace_rays(o, d, cfg, argb=argb)
    st = ds.last_trace_stats
    hit = planes["hit_id"] >= 0
    n_id = int((got.id != planes["hit_id"]).sum())
    n_t = int((_bits(got.t[hit]) != _bits(planes["hit_t"][hit])).sum())
    n_rgb = int((_bits(got.rgb[hit]) != _bits(planes["rgb"][hit])).any(axis=1).sum())
    n_argb = int((argb != buf.buffer).sum())
    print(f"{scene} {features}: {o.shape[0]} rays, hit share {hit.mean():.3f}; id diffs {n_id}, t bit diffs {n_t}, rgb bit diffs {n_rgb}, "
          f"argb diffs {n_argb}; batch {st['kernel_ms']:.3f} ms, frame {frame_stats['kernel_ms']:.3f} ms")
    assert hit.any() and (~hit).any()
    assert n_id == 0, np.flatnonzero(got.id != planes["hit_id"])[:10]
    assert np.array_equal(got.valid, hit)
    assert n_t == 0 and np.all(np.isposinf(got.t[~hit]))
    assert n_rgb == 0, np.flatnonzero((_bits(got.rgb) != _bits(planes["rgb"])).any(axis=1) & hit)[:10]
    assert np.all(got.rgb[~hit] == 0.0)
    assert n_argb == 0 and np.all(argb[~hit] == fill)
    for k in tr.COUNTERS:
        assert st[k] == frame_stats[k], (k, st[k], frame_stats[k])
    assert st["rays_traced"] == st["rays_primary"] + st["rays_reflection"] + st["rays_refraction"]


# ---- arbitrary rays equal the wrapper --------------------------------------------------------------------------------------
FEATURES = ([], ["soft_shadows"], ["realistic"], ["realistic", "soft_shadows"])
N_RAYS = {"test_scene": 20000, "text_lowres": 5000, "spheres": 20000, "empty": 4096}
CASES = [(s, f, False) for s in N_RAYS for f in FEATURES] + [("test_scene", ["realistic", "soft_shadows"], True)]


@pytest.mark.parametrize("name,features,cull", CASES)
def test_arbitrary_rays_equal_the_oracle(ref, name, features, cull):
    """All eight kinds of ray_query_cases.rays through process_ray: valid and id equal, t bit-exact, |dRGB| <= 1e-4 with no
    ray excluded, counters equal."""
    flat, ds = _scene(name)
    cfg = RenderConfig.from_features(list(features) + (["backface_culling"] if cull else []), n_cloud_sets=64)
    assert cfg.has("backface_culling") == cull
    o, d = rq.rays(flat, N_RAYS[name], seed=21 + list(N_RAYS).index(name))
    got = ds.trace_rays(o, d, cfg)
    want = tr.ref_trace(ref, flat, cfg, o, d)
    tr.check_against_ref(got, ds.last_trace_stats, want, what=f"{name} {features} cull={cull}")
    if flat.n_objects:
        assert want["valid"].mean() > 0.2, "too few valid rays to say anything"


# ---- edge cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", [[], ["realistic"]])
def test_dead_rays_null_planes_and_misses(features):
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(features)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    good_o, good_d = np.float32([0.5, 0.4, 0.0]), np.float32([0.0, 0.0, 1.0])
    o = np.array([good_o] * 9, np.float32)
    d = np.array([good_d] * 9, np.float32)
    d[0] = 0.0
    d[1, 0] = nan
    d[2, 1] = inf
    d[3, 2] = -inf
    o[4, 0] = inf
    o[5, 1] = nan
    o[6, 2] = -inf
    d[7] = (0.0, 0.0, -1.0)  # a live ray that leaves the scene: a miss
    argb = np.full(9, 0xABCDEF01, np.uint32)
    got = ds.trace_rays(o, d, cfg, argb=argb)
    st = ds.last_trace_stats
    assert (got.id[:8] == -1).all() and np.isposinf(got.t[:8]).all() and not got.valid[:8].any() and (got.rgb[:8] == 0).all()
    assert (argb[:8] == 0xABCDEF01).all(), "a miss must leave argb untouched"
    assert got.valid[8] and got.id[8] >= 0 and np.isfinite(got.t[8]) and argb[8] >> 24 == 0xFF
    assert st["rays_primary"] == 2 and st["pixels_written"] == 1, st  # the seven dead rays are not counted
    # NULL planes are not written: only `id` (then only `rgb`) is asked for, the neighbouring memory is a sentinel
    lib = _lib.load()
    p, keep = _abi.make_params(cfg)
    b = _abi.rt_ray_batch(_abi.RT_ABI_VERSION, 9, o.ctypes.data, d.ctypes.data, None, 0)
    ids = np.full(11, 12345, np.int32)
    _lib.check(lib.rt_trace_rays(ds.handle, C.byref(p), C.byref(b), C.byref(_abi.rt_ray_radiance(None, None, ids[1:].ctypes.data, None, None)), None))
    assert ids[0] == 12345 and ids[10] == 12345 and np.array_equal(ids[1:10], got.id)
    rgb = np.full((11, 3), 7.0, np.float32)
    _lib.check(lib.rt_trace_rays(ds.handle, C.byref(p), C.byref(b), C.byref(_abi.rt_ray_radiance(rgb[1:].ctypes.data, None, None, None, None)), None))
    assert (rgb[0] == 7.0).all() and (rgb[10] == 7.0).all() and np.array_equal(_bits(rgb[1:10]), _bits(got.rgb))
    # n_rays = 0 is a no-op
    b.n_rays = 0
    st0 = _abi.rt_stats()
    _lib.check(lib.rt_trace_rays(ds.handle, C.byref(p), C.byref(b), C.byref(_abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)), C.byref(st0)))
    assert ids[0] == 12345 and st0.rays_primary == 0
    # the anti-aliasing bit is refused, whatever else is right
    p.flags |= _abi.RT_FLAG_ANTI_ALIASING
    b.n_rays = 9
    assert lib.rt_trace_rays(ds.handle, C.byref(p), C.byref(b), C.byref(_abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)), None) == _abi.RT_ERR_INVALID_ARG


def test_a_batch_of_2_24_plus_17_rays(ref):
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features([])
    n = (1 << 24) + 17
    rng = np.random.default_rng(3)
    lo, hi = rq.bounds(flat)
    o = (lo + rng.random((n, 3), np.float32) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((n, 3), np.float32)
    got = ds.trace_rays(o, d, cfg)
    st = ds.last_trace_stats
    sel = np.concatenate([np.arange(0, n, 997), [n - 2, n - 1]]).astype(np.uint32)
    want = tr.ref_trace(ref, flat, cfg, o[sel], d[sel], index=sel)
    sub = type(got)(got.rgb[sel], got.valid[sel], got.id[sel], got.t[sel])
    tr.check_against_ref(sub, None, want, what=f"2^24 + 17 rays, {sel.size} sampled")
    assert st["rays_primary"] == n and st["pixels_written"] == int(got.valid.sum()), st
    print(f"2^24 + 17 rays: {st['kernel_ms']:.2f} ms on the device, {st['total_ms']:.1f} ms with staging")


# ---- every batch is verified -----------------------------------------------------------------------------------------------
def _wall_and_glass():
    """A matte wall on the left, metallic glass on the right (a slab and spheres): a hit on the glass has two children."""
    cfg = RenderConfig.from_features(["realistic"], depth_override=3)
    SW, SH, SD = cfg.scene_width, cfg.scene_height, cfg.scene_depth
    TP = TransmissionProperties
    s = Scene.with_capacities(16)
    matte = Material.new(ColorType.new(0.6, 0.7, 0.5), 0.0, 0.0, TP.none())
    glass = Material.new(ColorType.new(0.9, 0.95, 1.0), 0.3, 0.2, TP.new(0.3, 1.5))
    for t in BoundedPlane.with_material(-Vec3.unit_z(), Vec3.new(SW * F(0.25), SH * F(0.5), SD * F(0.8)), Vec3.unit_y(), SW * F(0.5), SH,
                                        F(0.01) * SD, matte).to_basic_geometries():
        s.add_triangle(t)
    for t in BoundedPlane.with_material(-Vec3.unit_z(), Vec3.new(SW * F(0.75), SH * F(0.5), SD * F(0.8)), Vec3.unit_y(), SW * F(0.5), SH,
                                        F(0.05) * SD, glass).to_basic_geometries():
        s.add_triangle(t)
    for cx, cy in ((0.62, 0.3), (0.88, 0.3), (0.62, 0.7), (0.88, 0.7)):
        s.add_sphere(SphereData.with_material(Vec3.new(SW * F(cx), SH * F(cy), SD * F(0.45)), F(0.11) * SD, glass))
    s.add_light(PointLight.new(Vec3.new(SW * F(0.5), SH * F(0.1), SD * F(0.02)), ColorType.new(1.0, 0.9, 0.8), 0.8).into())
    s.add_light(PointLight.new(Vec3.new(SW * F(0.2), SH * F(0.8), SD * F(0.1)), ColorType.new(0.7, 0.8, 1.0), 0.5).into())
    return cfg, s.flatten()


def _aimed(cfg, x0, x1, n, seed):
    """n rays from the reference's focus towards a grid of points x0 .. x1 (fractions of the scene width) on the plane
    z = 0.8 depth, in raster order (neighbours in the batch are neighbours in space)."""
    w = 512
    h = n // w
    xs = (x0 + (x1 - x0) * (np.arange(w) + 0.5) / w) * float(cfg.scene_width)
    ys = (0.05 + 0.9 * (np.arange(h) + 0.5) / h) * float(cfg.scene_height)
    X, Y = np.meshgrid(xs, ys)
    tgt = np.stack([X.ravel(), Y.ravel(), np.full(n, 0.8 * float(cfg.scene_depth))], axis=1)
    f = cfg.focus
    o = np.broadcast_to(np.array([float(f.x), float(f.y), float(f.z)]), tgt.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(tgt - o, np.float32)


def test_every_batch_is_verified(ref):
    """Batch A (2^17 rays at the matte wall: no children) leaves queues sized for a batch without children; batch B (2^17
    rays at the glass, depth 3: two children per hit) has the same shape and needs more.  B is right -- colours and
    counters equal the wrapper's -- because it was verified and run again, which the growth of the queues shows."""
    cfg, flat = _wall_and_glass()
    ds = DeviceScene(flat, 0)
    n = 1 << 17
    oa, da = _aimed(cfg, 0.02, 0.48, n, 1)
    ob, db = _aimed(cfg, 0.52, 0.98, n, 2)
    a = ds.trace_rays(oa, da, cfg)
    st_a = ds.last_trace_stats
    assert a.valid.all() and st_a["rays_reflection"] == 0 and st_a["rays_refraction"] == 0, st_a
    tr.check_against_ref(a, st_a, tr.ref_trace(ref, flat, cfg, oa, da), what="batch A (wall)")
    b = ds.trace_rays(ob, db, cfg)
    st_b = ds.last_trace_stats
    print(f"queue bytes: after A {st_a['queue_bytes']}, after B {st_b['queue_bytes']}; B: {st_b['rays_reflection']} reflection + "
          f"{st_b['rays_refraction']} refraction rays for {st_b['rays_primary']} primary")
    want = tr.ref_trace(ref, flat, cfg, ob, db)
    assert want["counters"]["rays_reflection"] + want["counters"]["rays_refraction"] > 2 * n, "batch B must overflow queues sized for A"
    tr.check_against_ref(b, st_b, want, what="batch B (glass)")
    assert st_a["queue_bytes"] > 0 and st_b["queue_bytes"] > st_a["queue_bytes"], (st_a["queue_bytes"], st_b["queue_bytes"])
    assert not (st_b["notes"] & _abi.RT_NOTE_FRAME_DROPPED_WORK)
    # ... and A again on the grown queues, then B again: the same bits both times
    a2 = ds.trace_rays(oa, da, cfg)
    b2 = ds.trace_rays(ob, db, cfg)
    for x, y in ((a, a2), (b, b2)):
        assert np.array_equal(_bits(x.rgb), _bits(y.rgb)) and np.array_equal(x.id, y.id) and np.array_equal(_bits(x.t), _bits(y.t))
    ds.close()


# ---- render state survives ---------------------------------------------------------------------------------------------------
def test_frames_and_batches_alternate_on_one_handle():
    cfg = RenderConfig.from_features(["anti_aliasing", "realistic", "soft_shadows"], n_cloud_sets=64)
    flat = scenes.test_scene(cfg).flatten()
    r = RaytracerRenderer(cfg, device=0)
    ds = r.device_scene(flat)
    o, d = rq.rays(flat, 60000, seed=33)
    frames, batches = [], []
    for _ in range(2):
        buf = ImageBuffer.new(cfg.width, cfg.height)
        planes = r.render(buf, flat, aux=True)
        assert not (r.last_stats["notes"] & _abi.RT_NOTE_FRAME_DROPPED_WORK), r.last_stats
        frames.append((buf.buffer.copy(), planes["rgb"].copy(), dict(r.last_stats)))
        batches.append((ds.trace_rays(o, d, cfg), dict(ds.last_trace_stats)))
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(_bits(frames[0][1]), _bits(frames[1][1]))
    (b0, s0), (b1, s1) = batches
    assert b0.valid.mean() > 0.2
    for k in ("rgb", "t"):
        assert np.array_equal(_bits(getattr(b0, k)), _bits(getattr(b1, k))), k
    assert np.array_equal(b0.id, b1.id) and np.array_equal(b0.valid, b1.valid)
    for k in tr.COUNTERS + ("rays_traced",):
        assert s0[k] == s1[k] and frames[0][2][k] == frames[1][2][k], k


# ---- camera render -----------------------------------------------------------------------------------------------------------
def test_render_camera_from_a_second_viewpoint(ref):
    cfg = RenderConfig.from_features(["realistic", "soft_shadows"], n_cloud_sets=64)
    flat = scenes.semesterbild(cfg, "text_lowres").flatten()
    SW, SH, SD = float(cfg.scene_width), float(cfg.scene_height), float(cfg.scene_depth)
    cam = camera.PinholeCamera(eye=(-0.45 * SW, 0.25 * SH, -1.1 * SD), target=(0.5 * SW, 0.5 * SH, 0.6 * SD), up=(0.0, -1.0, 0.0),
                               fov_y_deg=38.0, width=640, height=480)
    r = RaytracerRenderer(cfg, device=0)
    fill = 0xFF202020
    buf = ImageBuffer.new_with_color(cam.width, cam.height, fill)
    out = r.render_camera(buf, flat, cam)
    assert out.valid.mean() >= 0.3, out.valid.mean()
    assert np.all(buf.buffer[~out.valid] == fill) and np.all(buf.buffer[out.valid] >> 24 == 0xFF)
    assert r.last_stats["pixels_written"] == int(out.valid.sum())
    o, d = cam.rays()
    sel = np.arange(11, o.shape[0], 101).astype(np.uint32)
    want = tr.ref_trace(ref, flat, cfg, o[sel], d[sel], argb_fill=fill, index=sel)
    sub = type(out)(out.rgb[sel], out.valid[sel], out.id[sel], out.t[sel])
    tr.check_against_ref(sub, None, want, what=f"second viewpoint, {sel.size} of {o.shape[0]} rays")
    # the packed pixels: the wrapper's quantisation of ITS colour; a colour within 1e-4 can round to the neighbouring byte
    dq = np.abs(((buf.buffer[sel][:, None] >> np.array([16, 8, 0])) & 0xFF).astype(int) - ((want["argb"][:, None] >> np.array([16, 8, 0])) & 0xFF).astype(int))
    assert dq.max() <= 1 and np.array_equal(buf.buffer[sel] >> 24, want["argb"] >> 24)


# ---- torch device tensors ------------------------------------------------------------------------------------------------------
# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no
# GPU): the test that hands tensors to the library runs in a child process of its own
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_trace_rays_gpu as T
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


def test_device_entry_point_with_torch_tensors():
    """rt_trace_rays_device on a non-default stream gives the bits of the host entry point; bad tensors raise."""
    _run_child("device_entry_point_with_torch_tensors")


def device_entry_point_with_torch_tensors():
    import torch

    flat, ds = _scene("test_scene")
    o, d = rq.rays(flat, 40000, seed=5)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    for features in ([], ["soft_shadows"], ["realistic", "soft_shadows"]):
        cfg = RenderConfig.from_features(features, n_cloud_sets=64)
        argb_h = np.full(o.shape[0], 0x11223344, np.uint32)
        host = ds.trace_rays(o, d, cfg, argb=argb_h)
        host_stats = ds.last_trace_stats
        with torch.cuda.stream(s):
            to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
            argb_t = torch.full((o.shape[0],), 0x11223344, dtype=torch.int32, device=dev)
            got = ds.trace_rays(to, td, cfg, argb=argb_t)
        s.synchronize()
        assert isinstance(got.rgb, torch.Tensor) and got.rgb.device == dev and got.valid.dtype == torch.bool
        for k in ("rgb", "valid", "id", "t"):
            assert np.array_equal(_bits(getattr(got, k).cpu().numpy()), _bits(getattr(host, k))), (features, k)
        assert np.array_equal(argb_t.cpu().numpy().view(np.uint32), argb_h), features
        st = _abi.rt_stats()
        _lib.check(_lib.load().rt_render_collect_stats(ds.handle, C.byref(st)))
        for k in tr.COUNTERS + ("rays_traced",):
            assert getattr(st, k) == host_stats[k], (features, k)
    cfg = RenderConfig.from_features([])
    with pytest.raises(ValueError):
        ds.trace_rays(to.double(), td.double(), cfg)
    with pytest.raises(ValueError):
        ds.trace_rays(to.cpu(), td.cpu(), cfg)
    with pytest.raises(ValueError):
        ds.trace_rays(to[:, :2], td[:, :2], cfg)
    with pytest.raises(ValueError):
        ds.trace_rays(to, td[:-1], cfg)
    with pytest.raises(ValueError):
        ds.trace_rays(to, td, cfg, argb=argb_t.long())
