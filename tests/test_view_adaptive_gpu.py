"""Adaptive camera views on the GPU (rt_view_enable_adaptive, rt_render_view_adaptive*): the mask against the host model of
the rule; the frame against where(mask, the full view, the plane_of == 0 resolve of the one-sample view), both rendered by the
existing rt_render_view on the same scene and shading, array_equal on every plane; the counters; views in use -- a camera
that moves, a scene that is updated, an ordinary frame after an adaptive one; the device forms with torch tensors; the
refusals that need a view; the C example; and the partition primitive on its own, through a probe linked against the library.

The base planes (what pass 1 wrote) stay inside the view.  The frame of a ONE-sample view with the table's sample 0 holds the
same rays with the same batch indices -- hence the same light-cloud keys -- traced by the same kernels, and a ray's result does
not depend on what shares its wavefront: it stands for the base planes here, and the id and t planes of the adaptive frame,
which ARE the base planes', are compared with it bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, Refine, _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceView

import scene_update_cases as su
import view_adapt_cases as va
import view_cases as vc
from test_scene_pack_host import CSRC, HIPCC, ROOT
from test_scene_update_kernels_gpu import hip_ok

gpu = pytest.mark.gpu
ORDERS = ("none", "once", "always")
PLANES = ("rgb", "valid", "id", "t")
_cache = {}


def _scene():
    if "ds" not in _cache:
        _cache["ds"] = DeviceScene(va.scene_flat(), 0)
    return _cache["ds"]


def rule(criteria=va.DEPTH | va.COLOUR):
    return Refine(criteria=criteria, colour_tol=va.COLOUR_TOL, depth_tol=va.DEPTH_TOL)


def planes(r, argb):
    out = {k: np.asarray(getattr(r, k)) for k in PLANES}
    out["valid"] = out["valid"].astype(bool)
    out["argb"] = argb
    return out


def references(ds, cfg, w, h, smp, cam, order="once"):
    """rt_render_view of the full view and of the one-sample view -> (full planes, plane-0 planes, the plane_of == 0 resolve)"""
    views = [DeviceView(0, w, h, s, order=order, camera=cam) for s in (smp, smp[:1])]
    a_full, a_one = np.full(w * h, vc.FILL, np.uint32), np.full(w * h, vc.FILL, np.uint32)
    full = planes(ds.render_view(views[0], cfg, argb=a_full), a_full)
    one = planes(ds.render_view(views[1], cfg, argb=a_one), a_one)
    for v in views:
        v.close()
    flat = vc.resolve_model(w * h, smp.shape[0], np.zeros(smp.shape[0], np.uint8), one)
    return full, one, flat


def check_frame(label, got, mask, info, st, w, h, smp, rf, full, one, flat):
    n = w * h
    nd = vc.brute_dedup(smp)[1]
    want_mask, n_refined = va.refine_model(w, h, rf.struct(), one)
    mask = np.asarray(mask).astype(bool)
    print(f"{label}: {int(mask.sum())} of {n} refined (model {n_refined}); mask differs in {int((mask != want_mask).sum())}; info {info}; "
          f"rays_primary {st and st['rays_primary']}")
    assert np.array_equal(mask, want_mask), label
    assert info["n_refined"] == int(mask.sum()) == n_refined and info["n_live_rays"] == n_refined * (nd - 1), label
    if st is not None:
        # every ray of these cameras is live: plane 0 and the refined pixels' other planes
        assert st["rays_primary"] == n + n_refined * (nd - 1), (label, st["rays_primary"])
    want = va.where_pixels(mask, full, flat)
    vc.assert_pixels_equal(got, want, label)
    assert np.array_equal(got["argb"], want["argb"]) and np.all(got["argb"][~want["valid"]] == vc.FILL), label
    return mask


# ---- the frame ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("features,kw", va.SHADINGS)
def test_adaptive_frame_is_the_full_view_where_refined_and_sample_0_elsewhere(features, kw, order):
    """direct light and soft shadows, both camera kinds, the tables repeats9 / config16 / repeats24, every order mode, two frames
    each (the second reuses the order and its plane-0 part in mode "once")"""
    ds = _scene()
    cfg = RenderConfig.from_features(features, **kw)
    rf = rule()
    for what, w, h, smp, cam in va.views():
        full, one, flat = references(ds, cfg, w, h, smp, cam)
        view = DeviceView(0, w, h, smp, order=order, camera=cam).enable_adaptive()
        for frame in range(2):
            argb = np.full(w * h, vc.FILL, np.uint32)
            got = ds.render_view(view, cfg, argb=argb, refine=rf)
            mask = check_frame(f"{features} order={order} {what} frame {frame}", planes(got, argb), got.mask, view.adaptive_info,
                               ds.last_trace_stats, w, h, smp, rf, full, one, flat)
            assert 0.05 <= mask.mean() <= 0.95
        assert view.info["order_built"] == (order != "none")
        view.close()


@gpu
def test_every_gives_the_full_view_and_no_criterion_gives_sample_0():
    """RT_REFINE_EVERY: rt_render_view's frame; criteria == 0: the plane_of == 0 frame; ID alone; a one-sample table, which has no
    second pass"""
    ds = _scene()
    cfg = RenderConfig.from_features(["soft_shadows"], **va.SOFT)
    for what, w, h, smp, cam in va.views()[:2]:
        full, one, flat = references(ds, cfg, w, h, smp, cam)
        view = DeviceView(0, w, h, smp, camera=cam).enable_adaptive()
        for crit in (va.EVERY, 0, va.ID, va.EVERY | va.COLOUR):
            argb = np.full(w * h, vc.FILL, np.uint32)
            got = ds.render_view(view, cfg, argb=argb, refine=rule(crit))
            mask = check_frame(f"{what} criteria {crit}", planes(got, argb), got.mask, view.adaptive_info, ds.last_trace_stats, w, h, smp,
                               rule(crit), full, one, flat)
            if crit & va.EVERY:
                assert mask.all()
                vc.assert_pixels_equal(planes(got, argb), full, "every")
            if crit == 0:
                assert not mask.any()
                vc.assert_pixels_equal(planes(got, argb), flat, "none")
        view.close()
        single = DeviceView(0, w, h, smp[:1], camera=cam).enable_adaptive()
        argb = np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(single, cfg, argb=argb, refine=rule())
        assert single.adaptive_info["n_live_rays"] == 0 and ds.last_trace_stats["rays_primary"] == w * h
        vc.assert_pixels_equal(planes(got, argb), one, f"{what} one sample")
        assert np.array_equal(argb, one["argb"])
        assert np.array_equal(np.asarray(got.mask).astype(bool), va.refine_model(w, h, rule().struct(), one)[0])
        single.close()


@gpu
@pytest.mark.parametrize("what", va.REALISTIC_VIEWS)
def test_adaptive_frame_with_reflections_and_refractions(what):
    """the traces block and are verified at their end, twice; same equality, same counters"""
    ds = _scene()
    features, kw = va.REALISTIC
    cfg = RenderConfig.from_features(features, **kw)
    label, w, h, smp, cam = next(v for v in va.views() if v[0] == what)
    full, one, flat = references(ds, cfg, w, h, smp, cam)
    view = DeviceView(0, w, h, smp, camera=cam).enable_adaptive()
    argb = np.full(w * h, vc.FILL, np.uint32)
    got = ds.render_view(view, cfg, argb=argb, refine=rule())
    st = ds.last_trace_stats
    mask = check_frame(f"realistic {what}", planes(got, argb), got.mask, view.adaptive_info, st, w, h, smp, rule(), full, one, flat)
    assert 0.05 <= mask.mean() <= 0.95 and st["rays_reflection"] + st["rays_refraction"] > 0
    view.close()


# ---- views in use -----------------------------------------------------------------------------------------------------------------
@gpu
def test_a_moved_camera_a_scene_update_and_an_ordinary_frame_afterwards():
    """one adaptive view through its life: a frame; the camera moves (against a fresh view with that camera); the scene is
    updated (against a freshly created scene); then an ordinary rt_render_view on the same view equals a fresh view's frame"""
    flat0 = va.scene_flat()
    moved_scene = su.orbit_lights(su.move_spheres(flat0))
    cfg = RenderConfig.from_features(["soft_shadows"], **va.SOFT)
    what, w, h, smp, _ = va.views()[0]
    cam1 = vc.pinhole(w, h).view_camera()
    cam2 = vc.pinhole(w, h, eye=(0.62, 0.30, -1.4), target=(0.45, 0.5, 0.5)).view_camera()
    ds, fresh_ds = DeviceScene(flat0, 0), DeviceScene(moved_scene, 0)
    view = DeviceView(0, w, h, smp, camera=cam1).enable_adaptive().enable_adaptive()  # (idempotent)
    bytes_before = view.adaptive_info["bytes"]
    first = ds.render_view(view, cfg, refine=rule())
    view.set_camera(cam2)
    for scene, label in ((ds, "moved camera"), (fresh_ds, "updated scene")):
        if label == "updated scene":
            ds.update(moved_scene)
        fresh = DeviceView(0, w, h, smp, camera=cam2).enable_adaptive()
        a1, a2 = np.full(w * h, vc.FILL, np.uint32), np.full(w * h, vc.FILL, np.uint32)
        got = ds.render_view(view, cfg, argb=a1, refine=rule())
        st = dict(ds.last_trace_stats)
        want = scene.render_view(fresh, cfg, argb=a2, refine=rule())
        vc.assert_pixels_equal(planes(got, a1), planes(want, a2), label)
        assert np.array_equal(a1, a2) and np.array_equal(got.mask, want.mask) and 0 < np.asarray(got.mask).sum() < w * h, label
        full, one, flat = references(scene, cfg, w, h, smp, cam2)
        check_frame(label, planes(got, a1), got.mask, view.adaptive_info, st, w, h, smp, rule(), full, one, flat)
        fresh.close()
    assert (vc.bits(first.rgb) != vc.bits(got.rgb)).any(), "nothing moved"
    assert view.adaptive_info["bytes"] == bytes_before > 21 * w * h
    # an ordinary frame on the view that rendered adaptive ones: its per-ray planes and its order are whole again
    a1, a2 = np.full(w * h, vc.FILL, np.uint32), np.full(w * h, vc.FILL, np.uint32)
    plain = ds.render_view(view, cfg, argb=a1)
    fresh = DeviceView(0, w, h, smp, camera=cam2)
    want = ds.render_view(fresh, cfg, argb=a2)
    vc.assert_pixels_equal(planes(plain, a1), planes(want, a2), "ordinary frame after adaptive ones")
    assert np.array_equal(a1, a2)
    # and an adaptive frame after the ordinary one
    again = ds.render_view(view, cfg, refine=rule())
    vc.assert_pixels_equal({k: np.asarray(getattr(again, k)) for k in PLANES}, planes(got, None), "adaptive after ordinary")
    for x in (view, fresh, ds, fresh_ds):
        x.close()


@gpu
def test_render_camera_with_refine():
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import ImageBuffer, RaytracerRenderer

    w, h = vc.FRAMES[0]
    cfg = vc.frame_config(["anti_aliasing"], w, h)
    cam = vc.pinhole(w, h)
    r = RaytracerRenderer(cfg, device=0)
    buf, full_buf = ImageBuffer.new_with_color(w, h, vc.FILL), ImageBuffer.new_with_color(w, h, vc.FILL)
    got = r.render_camera(buf, va.scene_flat(), cam, samples="config", order=True, refine=rule())
    n_rays = r.last_stats["rays_primary"]
    full = r.render_camera(full_buf, va.scene_flat(), cam, samples="config", order=True)
    mask = np.asarray(got.mask).astype(bool)
    assert 0 < mask.sum() < w * h and n_rays < r.last_stats["rays_primary"]
    assert np.array_equal(vc.bits(np.asarray(got.rgb)[mask]), vc.bits(np.asarray(full.rgb)[mask]))
    assert np.array_equal(buf.buffer[mask], full_buf.buffer[mask])
    with pytest.raises(ValueError):
        r.render_camera(buf, va.scene_flat(), cam, refine=rule())


# ---- torch device tensors ------------------------------------------------------------------------------------------------------
# torch is imported BEFORE librt_hip.so is loaded, so the test that hands tensors to the library runs in a child process of
# its own, under its own time limit (as in tests/test_view_gpu.py)
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_view_adaptive_gpu as T
T.device_forms_with_torch_tensors()
print("CHILD-OK")
"""


@gpu
def test_device_forms_with_torch_tensors():
    """rt_render_view_adaptive_device, tensors on a non-default stream: every shading, view and order mode of the host-form test,
    two frames each, the same equality; the counters through rt_render_collect_stats are pass 2's alone"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def device_forms_with_torch_tensors():
    import torch

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    ds = _scene()
    rf = rule()
    for features, kw in va.SHADINGS:
        cfg = RenderConfig.from_features(features, **kw)
        for what, w, h, smp, cam in va.views():
            full, one, flat = references(ds, cfg, w, h, smp, cam)
            for order in ORDERS:
                view = DeviceView(0, w, h, smp, order=order, camera=cam).enable_adaptive()
                for frame in range(2):
                    with torch.cuda.stream(s):
                        targb = torch.full((w * h,), vc.FILL, dtype=torch.int32, device=dev)
                        got = ds.render_view(view, cfg, argb=targb, refine=rf)
                    s.synchronize()
                    assert isinstance(got.rgb, torch.Tensor) and got.rgb.device == dev and got.mask.dtype == torch.bool
                    host = {k: getattr(got, k).cpu().numpy() for k in PLANES}
                    host["valid"], host["argb"] = host["valid"].astype(bool), targb.cpu().numpy().view(np.uint32)
                    check_frame(f"{features} order={order} {what} device frame {frame}", host, got.mask.cpu().numpy(), view.adaptive_info, None, w, h, smp,
                                rf, full, one, flat)
                view.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_that_need_a_view():
    lib = _lib.load()
    ds = _scene()
    view = DeviceView(0, 8, 8, vc.sample_tables(_abi.RT_VIEW_PINHOLE)["repeats9"])
    p, keep = _abi.make_params(RenderConfig.from_features([]))
    buf = np.zeros((64, 3), np.float32)
    out = _abi.rt_ray_radiance(buf.ctypes.data, None, None, None, None)
    rf = va.refine()
    info = _abi.rt_view_adaptive_info()

    def refused(rc, part):
        msg = lib.rt_last_error().decode()
        assert rc == _abi.RT_ERR_INVALID_ARG and part in msg, (rc, msg)

    refused(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None), "no camera yet")
    view.set_camera(vc.pinhole(8, 8).view_camera())
    refused(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None), "rt_view_enable_adaptive")
    refused(lib.rt_render_view_adaptive_device(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None), "rt_view_enable_adaptive")
    refused(lib.rt_view_adaptive_read(view.handle, C.byref(info)), "rt_view_enable_adaptive")
    _lib.check(lib.rt_render_view(ds.handle, view.handle, C.byref(p), C.byref(out), None))  # an ordinary frame needs none
    view.enable_adaptive()
    _lib.check(lib.rt_view_adaptive_read(view.handle, C.byref(info)))
    assert info.n_refined == 0 and info.bytes > 0
    bad = va.refine(criteria=32)
    refused(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(bad), C.byref(out), None, None), "unknown criteria bits")
    _lib.check(lib.rt_render_view_adaptive(ds.handle, view.handle, C.byref(p), C.byref(rf), C.byref(out), None, None))  # mask and stats are optional
    view.close()


# ---- the C example ------------------------------------------------------------------------------------------------------------
def build_example(out_dir):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(str(out_dir), "c_view_adaptive_example")
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_view_adaptive_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe])
    return exe


def test_adaptive_example_links_against_the_abi(tmp_path):
    _lib.load()
    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mask 0110, 2 refined" in out.stdout
    assert "no HIP device" in out.stdout or "the mask equals the host model's mask" in out.stdout


@gpu
def test_adaptive_example_renders_on_the_gpu(tmp_path):
    out = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "the mask equals the host model's mask" in out.stdout and "every refined pixel equals the full frame's pixel" in out.stdout


# ---- the partition primitive ----------------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime.h>
#include "rt_internal.h"
#include "rt_ray_key.h"
#include "rt_view_adapt.h"
#define TRY(x)                                       \
  do {                                               \
    const hipError_t e_ = (x);                       \
    if (e_ != hipSuccess) return 1000 + (int)e_;     \
  } while (0)
extern "C" {
// perm_in[n] (NULL: the identity), flags[n] -> perm_out[n_out]; mask given (n_pixels entries): the flags are made on the device
// by rt_launch_view_flags (mask_mode 1: liveness, 2: ray < n_pixels) and returned in flags
int probe_partition(const uint32_t* perm_in, uint8_t* flags, uint32_t n, uint32_t n_out, uint32_t* perm_out, const uint8_t* mask,
                    uint32_t n_pixels, int mask_mode) {
  if (!n || n > (1u << 27) || n_out > n || (mask_mode && (!n_pixels || n_pixels > n))) return -100;
  TRY(hipSetDevice(0));
  const size_t n_counts = rt_partition_counts(n);
  uint32_t *d_in = nullptr, *d_out = nullptr, *counts = nullptr, *sums = nullptr;
  uint8_t *d_flags = nullptr, *d_mask = nullptr;
  int rc = 0;
  hipError_t e = hipSuccess;
  do {
    if ((e = hipMalloc(&d_flags, n)) != hipSuccess || (e = hipMalloc(&d_out, (size_t)(n_out ? n_out : 1) * 4)) != hipSuccess ||
        (e = hipMalloc(&counts, n_counts * 4)) != hipSuccess || (e = hipMalloc(&sums, RT_ORDER_SCAN_BLOCKS * 4)) != hipSuccess)
      break;
    if (perm_in && ((e = hipMalloc(&d_in, (size_t)n * 4)) != hipSuccess || (e = hipMemcpy(d_in, perm_in, (size_t)n * 4, hipMemcpyHostToDevice)) != hipSuccess))
      break;
    if ((e = hipMemset(d_out, 0xFF, (size_t)(n_out ? n_out : 1) * 4)) != hipSuccess || (e = hipMemset(counts, 0xFF, n_counts * 4)) != hipSuccess) break;
    if (mask_mode) {
      if ((e = hipMalloc(&d_mask, n_pixels)) != hipSuccess || (e = hipMemcpy(d_mask, mask, n_pixels, hipMemcpyHostToDevice)) != hipSuccess) break;
      if ((e = (hipError_t)rt_launch_view_flags(d_in, n, n_pixels, mask_mode == 1 ? d_mask : nullptr, d_flags, nullptr)) != hipSuccess) break;
    } else if ((e = hipMemcpy(d_flags, flags, n, hipMemcpyHostToDevice)) != hipSuccess) {
      break;
    }
    if ((e = (hipError_t)rt_launch_partition(d_in, d_flags, n, n_out, counts, sums, d_out, nullptr)) != hipSuccess) break;
    if ((e = hipDeviceSynchronize()) != hipSuccess) break;
    if ((e = hipMemcpy(perm_out, d_out, (size_t)n_out * 4, hipMemcpyDeviceToHost)) != hipSuccess) break;
    if ((e = hipMemcpy(flags, d_flags, n, hipMemcpyDeviceToHost)) != hipSuccess) break;
  } while (0);
  if (e != hipSuccess) return 1000 + (int)e;  // (nothing further is started on the device; the process ends with the test)
  for (void* p : {(void*)d_in, (void*)d_out, (void*)counts, (void*)sums, (void*)d_flags, (void*)d_mask})
    if (p) TRY(hipFree(p));
  return rc;
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("partition_probe")
    src, so = d / "probe.cpp", d / "probe.so"
    src.write_text(PROBE)
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    # none of the csrc sources: the launchers and their kernels come from the library under test
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_partition.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    return lib


def partition(probe, perm, flags, n_out=None, mask=None, n_pixels=0, mode=0):
    n = len(flags)
    n_out = n if n_out is None else n_out
    f = np.ascontiguousarray(flags).astype(np.uint8)
    out = np.full(max(n_out, 1), 0xFFFFFFFF, np.uint32)
    perm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    m = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)
    rc = probe.probe_partition(None if perm is None else perm.ctypes.data, f.ctypes.data, n, n_out, out.ctypes.data,
                               None if m is None else m.ctypes.data, n_pixels, mode)
    hip_ok(rc, "probe_partition")
    return out[:n_out], f.astype(bool)


def test_the_probe_builds_against_the_library_and_refuses_misuse(probe):
    """without a GPU: the probe links against the library's launchers and refuses sizes that would leave a buffer"""
    f = np.zeros(4, np.uint8)
    out = np.zeros(4, np.uint32)
    assert probe.probe_partition(None, f.ctypes.data, 0, 0, out.ctypes.data, None, 0, 0) == -100
    assert probe.probe_partition(None, f.ctypes.data, 4, 5, out.ctypes.data, None, 0, 0) == -100
    assert probe.probe_partition(None, f.ctypes.data, 4, 4, out.ctypes.data, f.ctypes.data, 5, 1) == -100


@gpu
@pytest.mark.parametrize("n", [1, 63, 256, 257, 1000, 4097, 70001])
def test_partition_equals_the_numpy_partition(probe, n):
    """all set, none set, one set (first, last, in the middle), random flags; the identity and a random permutation; a
    truncated output.  n: below a wavefront, one workgroup exactly, one entry more, no multiple of 256, several scan entries."""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.uint32)
    cases = [np.ones(n, bool), np.zeros(n, bool), rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.03]
    for k in sorted({0, n // 2, n - 1}):
        one = np.zeros(n, bool)
        one[k] = True
        cases.append(one)
    for flags in cases:
        for p in (None, perm):
            got, _ = partition(probe, p, flags)
            assert np.array_equal(got, va.partition_numpy(p, flags)), (n, int(flags.sum()), p is None)
    flags = cases[2]
    got, _ = partition(probe, perm, flags, n_out=n // 3)
    assert np.array_equal(got, va.partition_numpy(perm, flags, n // 3))


@gpu
def test_the_flag_kernels_and_the_partitions_of_a_frame(probe):
    """the two predicates of an adaptive frame, made on the device: liveness (plane >= 1 and mask) over the whole batch, and
    ray < n_pixels truncated to n_pixels entries -- a permutation of plane 0 in the order's order"""
    rng = np.random.default_rng(8)
    n_pix, nd = 37 * 29, 7
    n = n_pix * nd
    mask = rng.uniform(size=n_pix) < 0.4
    for perm in (None, rng.permutation(n).astype(np.uint32)):
        ident = np.arange(n, dtype=np.uint32) if perm is None else perm
        got, flags = partition(probe, perm, np.zeros(n, bool), mask=mask, n_pixels=n_pix, mode=1)
        want_flags = va.live_flags_numpy(ident, n_pix, mask)
        assert np.array_equal(flags, want_flags) and np.array_equal(got, va.partition_numpy(perm, want_flags))
        assert np.array_equal(np.sort(got), np.arange(n))
        got0, flags0 = partition(probe, perm, np.zeros(n, bool), n_out=n_pix, mask=mask, n_pixels=n_pix, mode=2)
        assert np.array_equal(flags0, ident < n_pix) and np.array_equal(got0, va.partition_numpy(perm, ident < n_pix, n_pix))
        assert np.array_equal(np.sort(got0), np.arange(n_pix))
