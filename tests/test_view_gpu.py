"""Camera views on the GPU (rt_view*, rt_render_view*): the generator against its host model, word for word; a view's frame
against the resolve model of a GPU trace of the model's rays, bit for bit in every order mode and through both entry
points; against the oracle-based CPU reference and against rt_render's own anti-aliased frame with the project's bars; and
what is particular to views -- a camera that moves, a scene that is updated, the refusals that need a view."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, sampling, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceView, ImageBuffer, RaytracerRenderer

import ray_query_cases as rq
import scene_update_cases as su
import trace_rays_cases as tr
import view_cases as vc

pytestmark = pytest.mark.gpu

W, H = vc.FRAMES[0]
SOFT = dict(n_cloud_sets=64)
_cache = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("viewref"))


def _flat(name):
    """test_scene (spheres + triangles + glass) framed for a W x H reference camera, its spheres alone, or nothing"""
    if name == "empty":
        return rq.scene("empty")[1]
    flat = scenes.test_scene(vc.frame_config([], W, H)).flatten().contiguous()
    return flat.without_triangles().contiguous() if name == "spheres" else flat


def _scene(name):
    if name not in _cache:
        flat = _flat(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _views():
    """the views most tests render, one per sample count of view_cases.sample_tables, both kinds and both frames among them:
    9 samples (sample 0 repeated in the second packet), 24 (20 distinct, three packets), 1 (taken unscaled), 7 (one packet with
    an empty lane, no `rest`) and the configuration's 16 (9 distinct).  The first is a pinhole over the scene's own frame."""
    wide, full = vc.frame_config([], 64, 4), vc.frame_config([], 37, 29)
    pin, ref_kind = _abi.RT_VIEW_PINHOLE, _abi.RT_VIEW_REFERENCE
    return [("pinhole 37x29 repeats9", 37, 29, vc.sample_tables(pin)["repeats9"], vc.pinhole(37, 29).view_camera()),
            ("reference 64x4 repeats24", 64, 4, vc.sample_tables(ref_kind, wide)["repeats24"], camera.reference_view_camera(wide)),
            ("pinhole 64x4 centre1", 64, 4, vc.sample_tables(pin)["centre1"], vc.pinhole(64, 4).view_camera()),
            ("reference 37x29 distinct7", 37, 29, vc.sample_tables(ref_kind, full)["distinct7"], camera.reference_view_camera(full)),
            ("pinhole 37x29 config16", 37, 29, vc.sample_tables(pin, full)["config16"], vc.pinhole(37, 29).view_camera())]


def _expected(ds, cfg, w, h, smp, cam):
    """resolve model of a GPU trace of the model's rays -> (pixel planes, the trace's stats)"""
    o, d, plane_of, nd = vc.model_rays(w, h, smp, cam)
    rays = ds.trace_rays(o, d, cfg)
    return vc.resolve_model(w * h, smp.shape[0], plane_of, rays), dict(ds.last_trace_stats)


# ---- the generator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(vc.KINDS))
def test_device_rays_equal_the_model(kind):
    """rt_view_rays (the kernel, staged) equals rt_view_rays_model in every word of origin and direction, for every sample table
    and both frames.  (rt_view_rays_device into tensors: device_forms_with_torch_tensors.)"""
    k = vc.KINDS[kind]
    for w, h in vc.FRAMES:
        cfg = vc.frame_config(["anti_aliasing"], w, h)
        cam = vc.view_camera(k, cfg, w, h)
        for name, smp in vc.sample_tables(k, cfg).items():
            o, d, plane_of, nd = vc.model_rays(w, h, smp, cam)
            view = DeviceView(0, w, h, smp, camera=cam)
            info = view.info
            go, gd = view.rays()
            n_o, n_d = int((vc.bits(go) != vc.bits(o)).sum()), int((vc.bits(gd) != vc.bits(d)).sum())
            print(f"{kind} {w}x{h} {name}: {info['n_rays']} rays of {nd} distinct samples, {info['bytes']} bytes; origin words differing {n_o}, direction {n_d}")
            assert info["n_distinct"] == nd and info["n_rays"] == nd * w * h == o.shape[0] and info["n_pixels"] == w * h
            assert np.array_equal(view.plane_of(), plane_of)
            assert n_o == 0 and n_d == 0
            view.close()


# ---- a view's frame is the resolve model of a GPU trace -------------------------------------------------------------------------
CASES = [("test_scene", [], {}), ("test_scene", ["soft_shadows"], SOFT), ("test_scene", ["realistic"], {}),
         ("spheres", ["realistic", "soft_shadows"], SOFT), ("empty", [], {})]


ORDERS = ("none", "once", "always")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene,features,kw", CASES)
def test_view_equals_the_resolve_model_of_a_gpu_trace(scene, features, kw, order):
    """rt_render_view (host planes) against rt_view_resolve_model(rt_trace_rays(model rays)): every pixel plane bit for bit, argb
    pre-filled and untouched where no sample hit, the trace's counters equal.  (rt_render_view_device:
    device_forms_with_torch_tensors, the same cases.)"""
    flat, ds = _scene(scene)
    cfg = RenderConfig.from_features(features, **kw)
    written = []
    for what, w, h, smp, cam in _views():
        want, want_stats = _expected(ds, cfg, w, h, smp, cam)
        written.append(float(want["valid"].mean()))
        view = DeviceView(0, w, h, smp, order=order, camera=cam)
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=argb)
        st = ds.last_trace_stats
        label = f"{scene} {features} order={order} {what}"
        print(f"{label}: {int(want['valid'].sum())} of {w * h} pixels written; stats {dict((k, st[k]) for k in tr.COUNTERS)}; view info {view.info}")
        vc.assert_pixels_equal(got, want, label)
        assert np.array_equal(argb, want["argb"]) and np.all(argb[~want["valid"]] == vc.FILL), label
        for k in tr.COUNTERS + ("rays_traced",):
            assert st[k] == want_stats[k], (label, k, st[k], want_stats[k])
        assert view.info["order_built"] == (order != "none")
        view.close()
    if scene == "empty":
        assert not want["valid"].any() and np.all(want["id"] == -1) and np.all(np.isposinf(want["t"]))
    else:
        assert 0.0 < written[0] < 1.0, "the pinhole frame should hold pixels that are written and pixels that are not"


# ---- torch device tensors ------------------------------------------------------------------------------------------------------
# torch is imported BEFORE librt_hip.so is loaded, so the test that hands tensors to the library runs in a child process of
# its own, under its own time limit (as in tests/test_ray_order_gpu.py)
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_view_gpu as T
T.device_forms_with_torch_tensors()
print("CHILD-OK")
"""


def test_device_forms_with_torch_tensors():
    """rt_view_rays_device and rt_render_view_device, tensors on a non-default stream: the model's rays, and for every case and
    order mode of the test above the resolve model of a GPU trace, bit for bit, two frames each (the second reuses the order in
    mode "once"), argb untouched where no sample hit, the trace's counters equal."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def device_forms_with_torch_tensors():
    import torch

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    for kind, k in sorted(vc.KINDS.items()):
        cfg = vc.frame_config(["anti_aliasing"], W, H)
        cam, smp = vc.view_camera(k, cfg, W, H), vc.sample_tables(k, cfg)["repeats9"]
        o, d, _, _ = vc.model_rays(W, H, smp, cam)
        view = DeviceView(0, W, H, smp, camera=cam)
        with torch.cuda.stream(s):
            to, td = view.rays(torch_device=True)
        s.synchronize()
        assert np.array_equal(vc.bits(to.cpu().numpy()), vc.bits(o)) and np.array_equal(vc.bits(td.cpu().numpy()), vc.bits(d)), kind
        view.close()
    lib = _lib.load()
    for scene, features, kw in CASES:
        flat, ds = _scene(scene)
        cfg = RenderConfig.from_features(features, **kw)
        for what, w, h, smp, cam in _views():
            want, want_stats = _expected(ds, cfg, w, h, smp, cam)
            for order in ORDERS:
                view = DeviceView(0, w, h, smp, order=order, camera=cam)
                for frame in range(2):
                    label = f"{scene} {features} order={order} {what} device frame {frame}"
                    with torch.cuda.stream(s):
                        targb = torch.full((w * h,), vc.FILL, dtype=torch.int32, device=dev)
                        got = ds.render_view(view, cfg, argb=targb)
                    s.synchronize()
                    assert isinstance(got.rgb, torch.Tensor) and got.rgb.device == dev
                    vc.assert_pixels_equal({k: getattr(got, k).cpu().numpy() for k in ("rgb", "valid", "id", "t")}, want, label)
                    assert np.array_equal(targb.cpu().numpy().view(np.uint32), want["argb"]), label
                    st = _abi.rt_stats()
                    _lib.check(lib.rt_render_collect_stats(ds.handle, C.byref(st)))
                    for k in tr.COUNTERS + ("rays_traced",):
                        assert getattr(st, k) == want_stats[k], (label, k)
                view.close()


# ---- against the CPU reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,features,kw", [c for c in CASES if c[0] != "empty"])
def test_view_against_the_cpu_reference(ref, scene, features, kw):
    """view_cases' resolve applied to trace_rays_cases.ref_trace with the view's indices (ray i keeps light-cloud key i), the
    bars of check_against_ref: valid and id equal, t bit-exact, |dRGB| <= 1e-4 with no pixel excluded, counters equal."""
    flat, ds = _scene(scene)
    cfg = RenderConfig.from_features(features, **kw)
    for what, w, h, smp, cam in _views():
        o, d, plane_of, nd = vc.model_rays(w, h, smp, cam)
        rays = tr.ref_trace(ref, flat, cfg, o, d, index=np.arange(o.shape[0], dtype=np.uint32))
        want = vc.resolve_model(w * h, smp.shape[0], plane_of, rays)
        want["counters"] = rays["counters"]
        view = DeviceView(0, w, h, smp, camera=cam)
        got = ds.render_view(view, cfg)
        tr.check_against_ref(got, ds.last_trace_stats, want, what=f"{scene} {features} {what}")
        view.close()


# ---- against rt_render ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", [["anti_aliasing"], ["anti_aliasing", "realistic"]])
def test_reference_view_against_rt_render(features):
    """The reference's camera with the configuration's sample table and light_mult == 1 is rt_render's anti-aliased frame:
    hit_id equal, hit_t bit-equal, |dRGB| <= 1e-4 against aux.rgb.  (Packed pixels are not compared bit for bit: rt_render
    sums in fixed point, so a channel may land on the other side of a rounding tie.)"""
    cfg = vc.frame_config(features, W, H)
    assert cfg.point_light_multiplicator == 1
    flat = scenes.test_scene(cfg).flatten().contiguous()
    r = RaytracerRenderer(cfg, device=0)
    buf = ImageBuffer.new(W, H)
    planes = r.render(buf, flat, aux=True)
    ds = r.device_scene(flat)
    view = DeviceView(0, W, H, sampling.aa_offsets(cfg), camera=camera.reference_view_camera(cfg))
    argb = np.zeros(W * H, np.uint32)
    got = ds.render_view(view, cfg, argb=argb)
    hit = planes["hit_id"] >= 0
    written = buf.buffer != 0
    err = np.abs(got.rgb.astype(np.float64) - planes["rgb"].astype(np.float64)).max(axis=1)
    chan = np.abs(((argb[:, None] >> np.array([16, 8, 0])) & 0xFF).astype(int) - ((buf.buffer[:, None] >> np.array([16, 8, 0])) & 0xFF).astype(int))
    print(f"{features}: {int(written.sum())} pixels written, id diffs {int((got.id != planes['hit_id']).sum())}, "
          f"t bit diffs {int((vc.bits(got.t[hit]) != vc.bits(planes['hit_t'][hit])).sum())}, max |dRGB| {err[written].max():.3e}, "
          f"packed channels differing {int((chan > 0).sum())} (largest step {int(chan.max())})")
    assert np.array_equal(got.id, planes["hit_id"])
    assert np.array_equal(vc.bits(got.t[hit]), vc.bits(planes["hit_t"][hit]))
    assert np.array_equal(got.valid, written)
    assert err[written].max() <= 1e-4
    view.close()
    ds.close()


# ---- views in use -----------------------------------------------------------------------------------------------------------------
def test_a_moved_camera_renders_what_a_fresh_view_renders():
    """rt_view_set_camera with a moved eye: the next frame equals a fresh view's frame with that camera, bit for bit, and the
    order built for the first camera is reused (no order time in the second frame)."""
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(["soft_shadows"], **SOFT)
    smp = vc.sample_tables(_abi.RT_VIEW_PINHOLE)["repeats9"]
    cam1 = vc.pinhole(W, H).view_camera()
    cam2 = vc.pinhole(W, H, eye=(0.62, 0.30, -1.4), target=(0.45, 0.5, 0.5)).view_camera()
    view = DeviceView(0, W, H, smp, camera=cam1)
    first = ds.render_view(view, cfg)
    info1 = view.info
    view.set_camera(cam2)
    a1 = np.full(W * H, vc.FILL, np.uint32)
    moved = ds.render_view(view, cfg, argb=a1)
    info2 = view.info
    fresh_view = DeviceView(0, W, H, smp, camera=cam2)
    a2 = np.full(W * H, vc.FILL, np.uint32)
    fresh = ds.render_view(fresh_view, cfg, argb=a2)
    print(f"order_ms first frame {info1['order_ms']:.3f}, second {info2['order_ms']:.3f}; rays_ms {info2['rays_ms']:.3f}, resolve_ms {info2['resolve_ms']:.3f}")
    vc.assert_pixels_equal(moved, {k: getattr(fresh, k) for k in ("rgb", "valid", "id", "t")}, "moved camera")
    assert np.array_equal(a1, a2)
    assert (vc.bits(first.rgb) != vc.bits(moved.rgb)).any(), "the camera did not move"
    assert info1["order_built"] and info1["order_ms"] > 0.0 and info2["order_ms"] == 0.0
    view.close()
    fresh_view.close()


def test_a_view_follows_a_scene_update():
    """after rt_scene_update the view's frame equals the frame of a freshly created scene, bit for bit"""
    flat = _flat("test_scene")
    moved = su.orbit_lights(su.move_spheres(flat))
    cfg = RenderConfig.from_features(["realistic"])
    what, w, h, smp, cam = _views()[0]
    ds, fresh = DeviceScene(flat, 0), DeviceScene(moved, 0)
    view = DeviceView(0, w, h, smp, camera=cam)
    before = ds.render_view(view, cfg)
    ds.update(moved)
    after = ds.render_view(view, cfg)
    want = fresh.render_view(view, cfg)
    vc.assert_pixels_equal(after, {k: getattr(want, k) for k in ("rgb", "valid", "id", "t")}, "updated scene")
    assert (vc.bits(before.rgb) != vc.bits(after.rgb)).any(), "the update changed nothing"
    view.close()
    ds.close()
    fresh.close()


def test_render_camera_with_samples_goes_through_a_view():
    """RaytracerRenderer.render_camera(samples="config"): the frame of a DeviceView with the configuration's table in pixels"""
    flat, _ = _scene("test_scene")
    cfg = vc.frame_config(["anti_aliasing"], W, H)
    cam = vc.pinhole(W, H)
    r = RaytracerRenderer(cfg, device=0)
    buf = ImageBuffer.new_with_color(W, H, vc.FILL)
    got = r.render_camera(buf, flat, cam, samples="config", order=True)
    ds = r.device_scene(flat)
    want, _ = _expected(ds, cfg, W, H, camera.view_samples(cfg, _abi.RT_VIEW_PINHOLE), cam.view_camera())
    vc.assert_pixels_equal(got, want, "render_camera")
    assert np.array_equal(buf.buffer, want["argb"]) and r.last_stats["rays_primary"] > 0
    ds.close()


def test_refusals_that_need_a_view():
    """A render and a ray generation before rt_view_set_camera are refused.  A view on another device than the scene is
    refused too, but that branch needs two devices to make the view on: with one visible device it does NOT run here, and
    no other test reaches it (the check follows the camera check in rt_view.cpp's check_render, before any HIP call)."""
    lib = _lib.load()
    flat, ds = _scene("test_scene")
    view = DeviceView(0, 8, 8)
    p, keep = _abi.make_params(RenderConfig.from_features([]))
    planes = np.zeros((64, 3), np.float32)
    out = _abi.rt_ray_radiance(planes.ctypes.data, None, None, None, None)

    def refused(rc, part):
        msg = lib.rt_last_error().decode()
        assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)

    refused(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None), "no camera yet")
    refused(lib.rt_render_view_device(ds.handle, view.handle, C.byref(p), C.byref(out), None), "no camera yet")
    refused(lib.rt_view_rays(view.handle, planes.ctypes.data, planes.ctypes.data), "no camera yet")
    view.set_camera(vc.pinhole(8, 8).view_camera())
    _lib.check(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None))
    if lib.rt_device_count() > 1:
        other = DeviceView(1, 8, 8, camera=vc.pinhole(8, 8).view_camera())
        refused(lib.rt_render_view(ds.handle, other.handle, C.byref(p), C.byref(out), None), "lives on device 1")
        other.close()
    view.close()


def test_view_example_renders_on_the_gpu(tmp_path):
    from test_view_host import build_example

    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "the frame equals the host models' frame" in out.stdout and "(reused)" in out.stdout
