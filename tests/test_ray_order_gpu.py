"""Ray orders on the GPU (rt_ray_order*, rt_trace_rays_ordered*).  An order changes which 64 rays share a wavefront and
nothing else, so every ordered call is held to the bits of the unordered call -- planes, argb, counters -- for every kind
of order; and not only to itself: ordered batches go through the oracle-based reference of the radiance tests as well.
The order a build produces is held to the host model (tests/ray_order_cases.py) bit for bit: its keys and, both sorts being
stable, its permutation.

Every test is one bounded piece of work in this process; the one test that needs torch runs in a child with a time limit
of its own, nothing is retried, and no child is started after one has ended abnormally."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib, camera, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RayOrder, RaytracerRenderer

import ray_order_cases as roc
import ray_query_cases as rq
import scene_update_cases as suc
import trace_rays_cases as tr

pytestmark = pytest.mark.gpu

_cache = {}
PLANES = ("rgb", "valid", "id", "t")
FILL = 0x00C0FFEE


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tr.build_ref(tmp_path_factory.mktemp("trref"))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return roc.build_probe(tmp_path_factory.mktemp("order_probe"))


def _scene(name):
    if name not in _cache:
        cfg, flat = rq.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _trace(ds, o, d, cfg, order):
    argb = np.full(o.shape[0], FILL, np.uint32)
    got = ds.trace_rays(o, d, cfg, argb=argb, order=order)
    return got, argb, dict(ds.last_trace_stats)


def _assert_same(a, b, what):
    (ga, argb_a, sa), (gb, argb_b, sb) = a, b
    for k in PLANES:
        x, y = _bits(getattr(ga, k)), _bits(getattr(gb, k))
        assert np.array_equal(x, y), (what, k, np.flatnonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[:10])
    assert np.array_equal(argb_a, argb_b), (what, "argb")
    for k in tr.COUNTERS + ("rays_traced",):
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])


def _orders(ds, o, d, seed):
    """the four kinds of order for one batch: built; built from a shuffled copy of the rays (a valid order of these rays
    all the same: it is a permutation) and reused; the caller's own, random; the caller's own, the identity"""
    n = o.shape[0]
    rng = np.random.default_rng(seed)
    sh = rng.permutation(n)
    return [("built", ds.ray_order(o, d)), ("built from a shuffle", ds.ray_order(o[sh], d[sh])),
            ("set random", RayOrder.from_permutation(0, rng.permutation(n))), ("set identity", RayOrder.from_permutation(0, np.arange(n)))]


SHADING = [([], False), (["soft_shadows"], False), (["realistic"], False), ([], True), (["soft_shadows"], True), (["realistic"], True)]


def _batches(flat):
    o_cam, d_cam = camera.reference_rays(RenderConfig.from_features([], width_override=384, height_override=320))
    o_all, d_all = rq.rays(flat, 20000, 21)
    out = [("camera rays", o_cam, d_cam), ("every kind of ray", o_all, d_all)]
    for n in (1, 255, 257, 1000):
        out.append((f"n = {n}", np.ascontiguousarray(o_all[3000:3000 + n]), np.ascontiguousarray(d_all[3000:3000 + n])))
    return out


# ---- bit equality with the unordered call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test_scene", "text_lowres"])
def test_ordered_calls_return_the_bits_of_the_unordered_call(name):
    flat, ds = _scene(name)
    n_checked = 0
    for what, o, d in _batches(flat):
        orders = _orders(ds, o, d, seed=o.shape[0])
        for features, cull in SHADING:
            cfg = RenderConfig.from_features(list(features) + (["backface_culling"] if cull else []), n_cloud_sets=64)
            plain = _trace(ds, o, d, cfg, None)
            if o.shape[0] > 1000:
                assert plain[0].valid.any() and not plain[0].valid.all(), "the batch needs hits and misses"
                assert np.all(plain[1][~plain[0].valid] == FILL), "a miss leaves argb"
            for kind, order in orders:
                _assert_same(plain, _trace(ds, o, d, cfg, order), f"{name} {what} {features} cull={cull} {kind}")
                n_checked += 1
            _assert_same(plain, _trace(ds, o, d, cfg, True), f"{name} {what} {features} cull={cull} built for the call")
        for _, order in orders:
            order.close()
    print(f"{name}: {n_checked} ordered batches equal their unordered call bit for bit")


def test_dead_rays_null_planes_and_empty_batches():
    flat, ds = _scene("test_scene")
    o, d = rq.rays(flat, 20000, 21)
    o, d = o.copy(), d.copy()
    d[5] = 0.0
    d[77, 0] = np.nan
    o[4000, 1] = np.inf
    cfg = RenderConfig.from_features(["soft_shadows"], n_cloud_sets=64)
    order = ds.ray_order(o, d)
    assert order.info["n_live"] == 20000 - 3 and set(order.permutation()[-3:].tolist()) == {5, 77, 4000}
    plain = _trace(ds, o, d, cfg, None)
    _assert_same(plain, _trace(ds, o, d, cfg, order), "dead rays")
    assert not plain[0].valid[[5, 77, 4000]].any()
    # NULL planes are not written: only `id` is asked for, its neighbours are sentinels
    lib = _lib.load()
    p, keep = _abi.make_params(cfg)
    n = o.shape[0]
    b = _abi.rt_ray_batch(_abi.RT_ABI_VERSION, n, o.ctypes.data, d.ctypes.data, None, 0)
    ids = np.full(n + 2, 12345, np.int32)
    st = _abi.rt_stats()
    _lib.check(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b), order.handle,
                                         C.byref(_abi.rt_ray_radiance(None, None, ids[1:].ctypes.data, None, None)), C.byref(st)))
    assert ids[0] == 12345 and ids[-1] == 12345 and np.array_equal(ids[1:-1], plain[0].id)
    assert st.rays_primary == plain[2]["rays_primary"] == n - 3
    # n_rays = 0: a no-op, with an order built for no rays or with none
    b0 = _abi.rt_ray_batch(_abi.RT_ABI_VERSION, 0, None, None, None, 0)
    _lib.check(lib.rt_ray_order_build(order.handle, C.byref(b0)))
    out = _abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)
    _lib.check(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b0), order.handle, C.byref(out), C.byref(st)))
    _lib.check(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b0), None, C.byref(out), C.byref(st)))
    assert ids[0] == 12345 and st.rays_primary == 0
    order.close()


# ---- not only against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", [["soft_shadows"], ["realistic"], ["realistic", "soft_shadows"]])
def test_ordered_rays_equal_the_oracle(ref, features):
    """The bars of the radiance tests on ORDERED batches: valid and id equal, t bit-exact, |dRGB| <= 1e-4 with no ray excluded,
    counters equal."""
    flat, ds = _scene("test_scene")
    cfg = RenderConfig.from_features(features, n_cloud_sets=64)
    o, d = rq.rays(flat, 20000, seed=21)
    want = tr.ref_trace(ref, flat, cfg, o, d)
    order = ds.ray_order(o, d)
    got = ds.trace_rays(o, d, cfg, order=order)
    tr.check_against_ref(got, ds.last_trace_stats, want, what=f"ordered {features}")
    got = ds.trace_rays(o, d, cfg, order=True)
    tr.check_against_ref(got, ds.last_trace_stats, want, what=f"ordered for the call {features}")
    assert want["valid"].mean() > 0.2
    order.close()


# ---- the device's order against the host model -------------------------------------------------------------------------------
def _against_model(probe, ds, o, d, origin_bits=0, what=""):
    n = o.shape[0]
    order = ds.ray_order(o, d, origin_bits=origin_bits)
    keys, perm, info = order.keys(), order.permutation(), order.info
    order.close()
    mkeys, mperm, minfo = roc.model(probe, o, d, origin_bits=origin_bits)
    n_key = int((keys != mkeys).sum())
    print(f"{what}: {n} rays, {info}; key diffs {n_key}")
    assert n_key == 0, np.flatnonzero(keys != mkeys)[:10]
    for k, v in minfo.items():
        assert info[k] == v, (k, info[k], v)
    assert info["bytes"] >= 20 * n
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), "not a permutation"
    sk = keys[perm]
    assert np.all(sk[1:] >= sk[:-1]), "keys[perm] decreases"
    assert np.array_equal(sk, mkeys[mperm])
    # each pass of the device's sort is stable and the model is std::stable_sort: rays of equal key stay in index order on both sides
    assert np.array_equal(perm, mperm), f"not the stable model's order, first at {np.flatnonzero(perm != mperm)[:5]}"
    return perm, mperm


def test_device_order_equals_the_host_model(probe):
    flat, ds = _scene("test_scene")
    o, d = rq.rays(flat, 20000, 21)
    o, d = o.copy(), d.copy()
    d[9] = 0.0
    o[11, 2] = np.nan
    _against_model(probe, ds, o, d, what="every kind of ray")
    for n in (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097):
        _against_model(probe, ds, o[:n], d[:n], what=f"n = {n}")
    W, H = 256, 192
    oc, dc = camera.reference_rays(RenderConfig.from_features([], width_override=W, height_override=H))
    perm, _ = _against_model(probe, ds, oc, dc, what="reference camera")
    hp = roc.half_perimeter(perm, W)
    op, dp = roc.pinhole(W, H).rays()
    perm, _ = _against_model(probe, ds, op, dp, what="pinhole")
    hp_p = roc.half_perimeter(perm, W)
    print(f"mean half-perimeter of the device's 64-ray runs: reference camera {hp:.2f}, pinhole {hp_p:.2f} (row-major 65.0)")
    assert hp <= 65.0 / 2 and hp_p <= 65.0 * 2 / 3
    # identical rays: one key; the stable order of equal keys is the identity, across wavefronts, rounds and a tile boundary
    perm, _ = _against_model(probe, ds, np.tile(o[:1], (5000, 1)), np.tile(d[:1], (5000, 1)), what="identical rays")
    assert np.array_equal(perm, np.arange(5000, dtype=np.uint32))


def test_device_order_of_2_22_plus_17_random_rays(probe):
    """1025 sort tiles, four passes; with three active origin axes and each bit split"""
    flat, ds = _scene("test_scene")
    n = (1 << 22) + 17
    o, d = roc.random_rays(n, seed=9)
    d[::100003] = 0.0  # a few dead rays
    for bits in (0, 10):
        _against_model(probe, ds, o, d, origin_bits=bits, what=f"2^22 + 17 random rays, origin_bits {bits}")


# ---- reuse -------------------------------------------------------------------------------------------------------------------
def test_an_order_survives_a_scene_update():
    flat = suc.flat_test_scene()
    ds = DeviceScene(flat, 0)
    cfg = RenderConfig.from_features(["realistic", "soft_shadows"], n_cloud_sets=64)
    o, d = rq.rays(flat, 20000, 21)
    order = ds.ray_order(o, d)
    before = _trace(ds, o, d, cfg, None)
    _assert_same(before, _trace(ds, o, d, cfg, order), "before the update")
    new = suc.move_spheres(suc.turn_mesh(suc.orbit_lights(flat), suc.mesh_range("test_scene", flat), 20.0))
    ds.update(new)
    after = _trace(ds, o, d, cfg, None)
    assert not np.array_equal(_bits(before[0].rgb), _bits(after[0].rgb)), "the update must change the picture"
    _assert_same(after, _trace(ds, o, d, cfg, order), "after the update")
    # ... and the order is not the scene's: another scene on the device reads it too
    fresh = DeviceScene(new, 0)
    _assert_same(after, _trace(fresh, o, d, cfg, order), "a fresh scene")
    fresh.close()
    order.close()
    ds.close()


def test_frames_and_ordered_batches_alternate_on_one_handle():
    cfg = RenderConfig.from_features(["anti_aliasing", "realistic", "soft_shadows"], n_cloud_sets=64)
    flat = scenes.test_scene(cfg).flatten()
    r = RaytracerRenderer(cfg, device=0)
    ds = r.device_scene(flat)
    o, d = rq.rays(flat, 60000, seed=33)
    plain = _trace(ds, o, d, cfg, None)
    order = ds.ray_order(o, d)
    frames, batches = [], []
    for k in range(2):
        buf = ImageBuffer.new(cfg.width, cfg.height)
        planes = r.render(buf, flat, aux=True)
        assert not (r.last_stats["notes"] & _abi.RT_NOTE_FRAME_DROPPED_WORK), r.last_stats
        frames.append((buf.buffer.copy(), planes["rgb"].copy(), dict(r.last_stats)))
        batches.append(_trace(ds, o, d, cfg, order if k == 0 else True))
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(_bits(frames[0][1]), _bits(frames[1][1]))
    for k in tr.COUNTERS + ("rays_traced",):
        assert frames[0][2][k] == frames[1][2][k], k
    assert plain[0].valid.mean() > 0.2
    for b in batches:
        _assert_same(plain, b, "between frames")
    order.close()


def test_render_camera_with_an_order():
    cfg = RenderConfig.from_features(["realistic", "soft_shadows"], n_cloud_sets=64)
    flat = scenes.semesterbild(cfg, "text_lowres").flatten()
    SW, SH, SD = float(cfg.scene_width), float(cfg.scene_height), float(cfg.scene_depth)
    cam = camera.PinholeCamera(eye=(-0.45 * SW, 0.25 * SH, -1.1 * SD), target=(0.5 * SW, 0.5 * SH, 0.6 * SD), up=(0.0, -1.0, 0.0),
                               fov_y_deg=38.0, width=640, height=480)
    r = RaytracerRenderer(cfg, device=0)
    bufs, outs, stats = [], [], []
    for order in (False, True):
        buf = ImageBuffer.new_with_color(cam.width, cam.height, 0xFF202020)
        outs.append(r.render_camera(buf, flat, cam, order=order))
        bufs.append(buf.buffer.copy())
        stats.append(dict(r.last_stats))
    assert outs[0].valid.mean() >= 0.3
    _assert_same((outs[0], bufs[0], stats[0]), (outs[1], bufs[1], stats[1]), "render_camera")


# ---- refusals that need a handle -----------------------------------------------------------------------------------------------
def test_handle_side_refusals():
    flat, ds = _scene("test_scene")
    lib = _lib.load()
    V = _abi.RT_ABI_VERSION
    cfg = RenderConfig.from_features([])
    p, keep = _abi.make_params(cfg)
    o, d = rq.rays(flat, 1000, 21)
    ids = np.zeros(1000, np.int32)
    out = _abi.rt_ray_radiance(None, None, ids.ctypes.data, None, None)
    b = _abi.rt_ray_batch(V, 1000, o.ctypes.data, d.ctypes.data, None, 0)

    def refused(rc, msg):
        err = lib.rt_last_error().decode()
        assert rc == _abi.RT_ERR_INVALID_ARG and msg in err, (rc, err)

    order = RayOrder(0, 1000)
    # never built or set
    refused(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None), "never been built")
    refused(lib.rt_trace_rays_ordered_device(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None), "never been built")
    refused(lib.rt_ray_order_read(order.handle, None, None, None), "never been built")
    # more rays than the capacity
    o2, d2 = rq.rays(flat, 1001, 21)
    refused(lib.rt_ray_order_build(order.handle, C.byref(_abi.rt_ray_batch(V, 1001, o2.ctypes.data, d2.ctypes.data, None, 0))), "capacity")
    ident = np.arange(1001, dtype=np.uint32)
    refused(lib.rt_ray_order_set(order.handle, ident.ctypes.data, 1001), "capacity")
    refused(lib.rt_ray_order_build(order.handle, C.byref(_abi.rt_ray_batch(V, 10, None, d.ctypes.data, None, 0))), "origin / direction")
    refused(lib.rt_ray_order_build(order.handle, C.byref(_abi.rt_ray_batch(3, 10, o.ctypes.data, d.ctypes.data, None, 0))), "abi_version")
    # not a permutation
    bad = np.arange(1000, dtype=np.uint32)
    bad[7] = 8
    refused(lib.rt_ray_order_set(order.handle, bad.ctypes.data, 1000), "appears twice")
    # a mismatched n
    _lib.check(lib.rt_ray_order_build(order.handle, C.byref(_abi.rt_ray_batch(V, 999, o.ctypes.data, d.ctypes.data, None, 0))))
    refused(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None), "holds 999 rays")
    refused(lib.rt_trace_rays_ordered_device(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None), "holds 999 rays")
    # a set order has no keys
    _lib.check(lib.rt_ray_order_set(order.handle, ident.ctypes.data, 1000))
    keys = np.zeros(1000, np.uint32)
    refused(lib.rt_ray_order_read(order.handle, None, keys.ctypes.data, None), "no keys")
    assert np.array_equal(order.permutation(), ident[:1000]) and order.info["n_live"] == 0
    # a progressive render owns the scene
    big = RenderConfig.from_features([])
    pp, keep2 = _abi.make_params(big)
    buf = np.zeros(big.width * big.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(pp), buf.ctypes.data, 64, C.byref(h)))
    rc = lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None)
    err = lib.rt_last_error().decode()
    rc2 = lib.rt_trace_rays_ordered_device(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None)
    err2 = lib.rt_last_error().decode()
    _lib.check(lib.rt_render_end(h, None))
    assert rc == rc2 == _abi.RT_ERR_INVALID_ARG and "progressive" in err and "progressive" in err2
    # ... and afterwards the same call goes through
    _lib.check(lib.rt_trace_rays_ordered(ds.handle, C.byref(p), C.byref(b), order.handle, C.byref(out), None))
    order.close()


# ---- torch device tensors ------------------------------------------------------------------------------------------------------
# torch is imported BEFORE librt_hip.so is loaded, so the test that hands tensors to the library runs in a child process of
# its own, under its own time limit; a child that ended abnormally is the last one started
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_ray_order_gpu as T
T.{name}()
print("CHILD-OK")
"""
_child_faulted = []


def _run_child(name):
    assert not _child_faulted, f"not started: {_child_faulted[0]} ended abnormally"
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        out = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here, name=name)],
                             capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _child_faulted.append(name)
        raise
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _child_faulted.append(name)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_device_entry_points_with_torch_tensors():
    """rt_ray_order_build_device + rt_trace_rays_ordered_device on a non-default stream give the bits of the host forms."""
    _run_child("device_entry_points_with_torch_tensors")


def device_entry_points_with_torch_tensors():
    import torch

    flat, ds = _scene("test_scene")
    o, d = rq.rays(flat, 40000, seed=5)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    host_order = ds.ray_order(o, d)
    for features in ([], ["soft_shadows"], ["realistic", "soft_shadows"]):
        cfg = RenderConfig.from_features(features, n_cloud_sets=64)
        argb_h = np.full(o.shape[0], 0x11223344, np.uint32)
        host = ds.trace_rays(o, d, cfg, argb=argb_h)
        host_stats = ds.last_trace_stats
        for kind in ("built on the stream", "built for the call", "a host-built order"):
            with torch.cuda.stream(s):
                to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
                argb_t = torch.full((o.shape[0],), 0x11223344, dtype=torch.int32, device=dev)
                order = {"built on the stream": lambda: ds.ray_order(to, td), "built for the call": lambda: True,
                         "a host-built order": lambda: host_order}[kind]()
                got = ds.trace_rays(to, td, cfg, argb=argb_t, order=order)
            s.synchronize()
            assert isinstance(got.rgb, torch.Tensor) and got.rgb.device == dev
            for k in PLANES:
                assert np.array_equal(_bits(getattr(got, k).cpu().numpy()), _bits(getattr(host, k))), (features, kind, k)
            assert np.array_equal(argb_t.cpu().numpy().view(np.uint32), argb_h), (features, kind)
            st = _abi.rt_stats()
            _lib.check(_lib.load().rt_render_collect_stats(ds.handle, C.byref(st)))
            for k in tr.COUNTERS + ("rays_traced",):
                assert getattr(st, k) == host_stats[k], (features, kind, k)
            if isinstance(order, RayOrder) and order is not host_order:
                # the stream-built order is the host-built one up to ties
                assert np.array_equal(order.keys(), host_order.keys())
                order.close()
    with pytest.raises(ValueError):
        ds.trace_rays(to, td, RenderConfig.from_features([]), order="yes")
    host_order.close()
