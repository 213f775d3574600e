"""In-place scene updates on the GPU (rt_scene_update / rt_scene_update_device, csrc/rt_update.hip): a handle that has been
updated renders and answers queries exactly as a handle freshly created from the updated description -- the invariant this
project already holds across traversals and knobs: the tree only prunes work, so a refitted tree gives the same bits as a
rebuilt one -- and both agree with the brute-force oracle within the existing bar (ids and t exact, |dRGB| <= RGB_TOL, equal
ray counters)."""
import ctypes as C
import types

import numpy as np
import pytest

import oracle_lib
import scene_update_cases as cases
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, ImageBuffer, RaytracerRenderer

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # the project's bar (tests/test_parity_gpu.py)
CONFIGS = {
    "direct": lambda: RenderConfig.from_features([]),
    "soft": lambda: RenderConfig.from_features(["anti_aliasing", "soft_shadows"], n_cloud_sets=64),
    "realistic": lambda: RenderConfig.from_features(["realistic"], depth_override=4),
}
SCENES = {"test_scene": cases.flat_test_scene, "semesterbild": cases.flat_semesterbild}
# oracle windows of the sizes the parity tests use, over the objects that move
WINDOWS = {"test_scene": (523, 163, 48, 32), "semesterbild": (194, 282, 32, 24)}
EVERYTHING = _abi.RT_UPDATE_INVALIDATES_RECEIVER_TABLES | _abi.RT_UPDATE_INVALIDATES_TILE_COSTS | _abi.RT_UPDATE_INVALIDATES_QUEUE_SIZES


def window_mask(cfg, win):
    m = np.zeros((cfg.height, cfg.width), bool)
    x0, y0, w, h = win
    m[y0:y0 + h, x0:x0 + w] = True
    return m.ravel()


def render(cfg, scene, win=None, renderer=None, **kw):
    """scene: a DeviceScene or a FlatScene -> (packed pixels, aux planes, stats)"""
    buf = ImageBuffer.new(cfg.width, cfg.height)
    r = renderer or RaytracerRenderer(cfg, device=0)
    planes = r.render(buf, scene, window=win, aux=True, **kw)
    return buf.buffer.copy(), planes, r.last_stats


def assert_same_frame(a, b, what):
    """packed pixels, hit ids and hit distances bit-equal on EVERY pixel; returns whether the float rgb planes are too"""
    assert np.array_equal(a[0], b[0]), f"{what}: {(a[0] != b[0]).sum()} packed pixels differ"
    assert np.array_equal(a[1]["hit_id"], b[1]["hit_id"]), f"{what}: hit ids differ"
    assert np.array_equal(a[1]["hit_t"].view(np.uint32), b[1]["hit_t"].view(np.uint32)), f"{what}: hit t differs"
    for k in ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written"):
        assert a[2][k] == b[2][k], (what, k, a[2][k], b[2][k])
    return np.array_equal(a[1]["rgb"].view(np.uint32), b[1]["rgb"].view(np.uint32))


def assert_matches_oracle(cfg, flat, win, got, what):
    """tests/test_parity_gpu.py's compare(), for a frame that has been rendered already"""
    argb_g, pg, sg = got
    argb_o, po, so = oracle_lib.render(flat, cfg, window=win)
    m = window_mask(cfg, win)
    assert np.array_equal(argb_g != 0, argb_o != 0), what
    assert not (argb_g[~m] != 0).any(), what
    assert np.array_equal(pg["hit_id"], po["hit_id"]), f"{what}: {(pg['hit_id'] != po['hit_id']).sum()} hit ids differ"
    hit = m & (po["hit_id"] >= 0)
    assert np.array_equal(pg["hit_t"][hit].view(np.uint32), po["hit_t"][hit].view(np.uint32)), f"{what}: hit t not bit-exact"
    d = np.abs(pg["rgb"] - po["rgb"]).max(axis=1)
    print(f"{what}: max |dRGB| vs oracle = {float(d.max()):.3e}, {int(hit.sum())} hit pixels, {len(np.unique(po['hit_id'][hit]))} objects")
    assert int((d > RGB_TOL).sum()) == 0, f"{what}: {(d > RGB_TOL).sum()} pixels exceed {RGB_TOL} (max {d.max():.3e})"
    for sh in (16, 8, 0):
        assert np.abs(((argb_g >> sh) & 0xFF).astype(np.int32) - ((argb_o >> sh) & 0xFF).astype(np.int32)).max() <= 1
    for k in ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written"):
        assert sg[k] == so[k], (what, k, sg[k], so[k])


# ---- 1. animation parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_animation_equals_fresh_handles_and_the_oracle(name, config):
    """Six scripted steps on ONE handle: light orbit, sphere move, mesh turn, 5 % jitter, material colours, back to the
    start.  After each the frame is bit-equal to the same frame of a handle created from that step's description, and
    within the bar of the oracle's."""
    cfg, win = CONFIGS[config](), WINDOWS[name]
    flat = SCENES[name]()
    ds = DeviceScene(flat, 0)
    first = render(cfg, ds, win)
    rgb_equal = []
    for label, step in cases.animation(name, flat):
        info = ds.update(step, info=True)
        assert info is not None and info["tables_invalidated"] & _abi.RT_UPDATE_INVALIDATES_QUEUE_SIZES
        got = render(cfg, ds, win)
        fresh_ds = DeviceScene(step, 0)
        fresh = render(cfg, fresh_ds, win)
        fresh_ds.close()
        what = f"{name} / {config} / {label}"
        rgb_equal.append(assert_same_frame(got, fresh, what))
        assert_matches_oracle(cfg, step, win, got, what)
        print(f"{what}: update {info['total_ms']:.3f} ms wall, {info['device_ms']:.3f} ms device, {info['nodes_refitted']} nodes, "
              f"{info['slots_rewritten']} slots, {info['receivers_disabled']} receivers disabled; float rgb bit-equal to fresh: {rgb_equal[-1]}")
    assert_same_frame(got, first, f"{name} / {config}: back at the start")
    print(f"{name} / {config}: float rgb planes bit-equal to a fresh handle's in {sum(rgb_equal)} of {len(rgb_equal)} steps")
    ds.close()


# ---- 2. identity --------------------------------------------------------------------------------------------------------------
def test_identity_update_changes_no_frame_and_reports_what_it_invalidates():
    cfg, win = CONFIGS["soft"](), WINDOWS["semesterbild"]
    flat = cases.flat_semesterbild()
    ds = DeviceScene(flat, 0)
    before = render(cfg, ds, win)
    assert ds.update(flat, info=True) is None, "an equal description is no call"
    lib = _lib.load()

    def send(groups):
        d, keep = _abi.make_scene_delta(flat, groups)
        info = _abi.rt_update_info()
        _lib.check(lib.rt_scene_update(ds.handle, C.byref(d), C.byref(info)))
        return info.as_dict()

    everything = _abi.scene_delta_groups(flat, flat, full=True)
    info = send(everything)
    assert info["tables_invalidated"] == EVERYTHING and info["nodes_refitted"] == ds.bvh_info()["n_nodes"]
    assert info["slots_rewritten"] == flat.n_triangles and info["receivers_disabled"] == 0
    assert info["device_ms"] > 0 and info["total_ms"] >= info["device_ms"] * 0.5
    after = render(cfg, ds, win)
    assert assert_same_frame(before, after, "identity"), "the float planes too"
    nothing = dict(spheres=False, triangles=None, materials=False, lights=False)
    info = send({**nothing, "materials": True})
    assert info["tables_invalidated"] == _abi.RT_UPDATE_INVALIDATES_QUEUE_SIZES and info["nodes_refitted"] == 0 and info["slots_rewritten"] == 0
    assert send({**nothing, "lights": True})["tables_invalidated"] == EVERYTHING
    assert send({**nothing, "spheres": True})["tables_invalidated"] == EVERYTHING
    assert assert_same_frame(before, render(cfg, ds, win), "identity, group by group")
    ds.close()


# ---- 3. every path sees the update --------------------------------------------------------------------------------------------
def rays_into(flat, n, seed):
    r = np.random.default_rng(seed)
    pts = np.concatenate([flat.sphere_center, flat.tri_v1, flat.tri_v1 + flat.tri_e1])
    lo, hi = pts.min(0), pts.max(0)
    o = r.uniform(lo, hi, (n, 3)) * [1, 1, 0] + [0, 0, lo[2] - 0.3 * (hi[2] - lo[2])]
    d = r.uniform(lo, hi, (n, 3)) - o
    return o.astype(np.float32), d.astype(np.float32)


def test_every_path_sees_the_update():
    name = "semesterbild"
    flat = SCENES[name]()
    turned = cases.animation(name, flat)[2][1]
    ds, fresh = DeviceScene(flat, 0), DeviceScene(turned, 0)
    o, d = rays_into(flat, 1 << 14, 3)
    before = ds.cast_rays(o, d)
    ds.update(turned)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    hits = ds.cast_rays(o, d)
    for a, b, field in zip(hits, fresh.cast_rays(o, d), hits._fields):
        assert np.array_equal(bits(a), bits(b)), f"cast_rays.{field}"
    assert not np.array_equal(bits(before.t), bits(hits.t)) and (hits.id >= 0).sum() > 1000, "the rays meet what moved"
    tmax = np.full(len(o), np.float32(2.0) * np.linalg.norm(d, axis=1).max().astype(np.float32))
    occ = ds.any_intersection(o, d, tmax)
    for a, b, field in zip(occ, fresh.any_intersection(o, d, tmax), occ._fields):
        if field == "color_filter":  # (unspecified where completely occluded)
            a, b = a[~occ.completely_occluded], b[~occ.completely_occluded]
        assert np.array_equal(bits(a), bits(b)), f"any_intersection.{field}"
    cfg = CONFIGS["realistic"]()
    rad = ds.trace_rays(o[:4096], d[:4096], cfg)
    for a, b, field in zip(rad, fresh.trace_rays(o[:4096], d[:4096], cfg), rad._fields):
        assert np.array_equal(bits(a), bits(b)), f"trace_rays.{field}"
    assert ds.last_trace_stats["rays_traced"] == fresh.last_trace_stats["rays_traced"]
    # a progressive render, and the union of two tile ranks
    cfg = CONFIGS["soft"]()
    r = RaytracerRenderer(cfg, device=0)
    bufs = []
    for scene in (ds, fresh):
        buf = ImageBuffer.new(cfg.width, cfg.height)
        r.render_progressive(buf, scene)
        bufs.append(buf.buffer.copy())
    assert np.array_equal(bufs[0], bufs[1]) and (bufs[0] != 0).any(), "render_progressive"
    whole = render(cfg, fresh)[0]
    assert np.array_equal(bufs[0], whole)
    union = np.zeros_like(whole)
    for rank in range(2):
        part = render(cfg, ds, n_ranks=2, rank=rank)[0]
        assert np.array_equal(part, render(cfg, fresh, n_ranks=2, rank=rank)[0]), f"rank {rank} of 2"
        assert not ((union != 0) & (part != 0)).any()
        union |= part
    assert np.array_equal(union, whole), "the two-tile-rank union"
    ds.close(), fresh.close()


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no
# GPU): the tests that hand tensors or torch streams to the library run in a child process of their own
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_scene_update_gpu as T
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
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 4. frames in flight ------------------------------------------------------------------------------------------------------
def test_update_waits_for_the_frames_in_flight():
    """two frames enqueued on two streams, then rt_scene_update without a synchronisation of the caller's: both frames show
    the old scene, the next one the new"""
    _run_child("update_waits_for_the_frames_in_flight")


def update_waits_for_the_frames_in_flight():
    import torch

    name = "semesterbild"
    cfg = CONFIGS["soft"]()
    flat = SCENES[name]()
    turned = cases.animation(name, flat)[2][1]
    old_frame, new_frame = render(cfg, flat)[0], render(cfg, turned)[0]
    assert not np.array_equal(old_frame, new_frame)
    lib = _lib.load()
    ds = DeviceScene(flat, 0)
    p, keep = _abi.make_params(cfg)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    fbs = [torch.zeros(cfg.width * cfg.height, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    for k in range(2):
        _lib.check(lib.rt_render_device(ds.handle, C.byref(p), C.c_void_p(fbs[k].data_ptr()), None, C.c_void_p(streams[k].cuda_stream)))
    d, keepd = _abi.make_scene_delta(turned, _abi.scene_delta_groups(flat, turned))
    _lib.check(lib.rt_scene_update(ds.handle, C.byref(d), None))
    _lib.check(lib.rt_render_device(ds.handle, C.byref(p), C.c_void_p(fbs[2].data_ptr()), None, C.c_void_p(streams[0].cuda_stream)))
    torch.cuda.synchronize(dev)
    got = [fb.cpu().numpy().view(np.uint32) for fb in fbs]
    assert np.array_equal(got[0], old_frame) and np.array_equal(got[1], old_frame), "the frames in flight show the old scene"
    assert np.array_equal(got[2], new_frame), "the next frame shows the new one"
    ds.close()


# ---- 5. soft-shadow tables ----------------------------------------------------------------------------------------------------
def test_soft_shadow_tables_keep_their_size_and_are_rebuilt():
    name = "semesterbild"
    cfg, win = CONFIGS["soft"](), (200, 150, 320, 240)
    flat = SCENES[name]()
    moved = cases.orbit_lights(flat)
    ds = DeviceScene(flat, 0, budget=2 << 30)  # (opted in: the per-cell candidate lists fit)
    render(cfg, ds, win)
    again = render(cfg, ds, win)
    mi = ds.memory_info()
    assert mi["n_receiver_cells"] > 0 and mi["cell_lists_built"] == 1 and mi["bytes_cell_lists"] > 0
    info = ds.update(moved, info=True)
    assert info["tables_invalidated"] == EVERYTHING and info["nodes_refitted"] == 0
    mid = ds.memory_info()
    assert mid["n_receiver_cells"] == mi["n_receiver_cells"] and mid["cell_lists_built"] == 0
    got = render(cfg, ds, win)
    assert got[2]["setup_ms"] > 0.0, "the flags were rebuilt by this frame"
    after = ds.memory_info()
    assert after["n_receiver_cells"] == mi["n_receiver_cells"] and after["cell_lists_built"] == 1
    assert after["bytes_cell_lists"] == mi["bytes_cell_lists"] and after["bytes_flags"] == mi["bytes_flags"]
    fresh_ds = DeviceScene(moved, 0, budget=2 << 30)
    assert_same_frame(got, render(cfg, fresh_ds, win), "light move, lists on")
    print(f"setup_ms: steady frame {again[2]['setup_ms']:.3f}, frame after the light move {got[2]['setup_ms']:.3f}")
    ds.close(), fresh_ds.close()


# ---- 6. device form -----------------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form():
    """torch tensors on the device through rt_scene_update_device give the frames of the host form, step by step"""
    _run_child("device_form_equals_host_form")


def device_form_equals_host_form():
    import torch

    name = "test_scene"
    cfg, win = CONFIGS["soft"](), WINDOWS[name]
    flat = SCENES[name]()
    steps = cases.animation(name, flat)
    host, devf = DeviceScene(flat, 0), DeviceScene(flat, 0)
    dev = torch.device("cuda", 0)
    prev = flat
    for label, step in steps:
        host.update(step)
        groups = _abi.scene_delta_groups(prev, step)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        arrays, first = {}, 0
        if groups["spheres"]:
            arrays.update({k: t(getattr(step, k)) for k in _abi.SPHERE_GROUP})
        if groups["triangles"]:
            first, count = groups["triangles"]
            arrays.update({k: t(getattr(step, k)[first:first + count]) for k in _abi.TRIANGLE_GROUP})
        if groups["materials"]:
            arrays["materials"] = t(step.materials)
        if groups["lights"]:
            arrays["lights"] = t(step.lights)
        info = devf.update(types.SimpleNamespace(**arrays), info=True, tri_first=first)
        assert info is not None and info["device_ms"] > 0
        for k in ("tri_v1", "tri_normal", "sphere_center", "materials", "lights"):
            assert np.array_equal(getattr(devf.flat, k).view(np.uint32), getattr(step, k).view(np.uint32)), "the description it holds follows"
        assert assert_same_frame(render(cfg, devf, win), render(cfg, host, win), f"device form / {label}"), "float planes too"
        prev = step
    with pytest.raises(ValueError):
        devf.update(types.SimpleNamespace(tri_v1=torch.zeros((3, 3), device=dev)))
    with pytest.raises(ValueError):
        devf.update(types.SimpleNamespace(lights=torch.zeros((1, 7), device=dev)))
    host.close(), devf.close()


def test_renderer_updates_its_cached_scene_in_place():
    name = "test_scene"
    cfg, win = CONFIGS["realistic"](), WINDOWS[name]
    flat = SCENES[name]()
    plain, in_place = RaytracerRenderer(cfg, device=0), RaytracerRenderer(cfg, device=0, update_in_place=True)
    handles = set()
    for label, step in [("start", flat)] + cases.animation(name, flat):
        a, b = render(cfg, step, win, renderer=plain), render(cfg, step, win, renderer=in_place)
        assert_same_frame(a, b, f"update_in_place / {label}")
        handles.add(in_place.device_scene(step).handle.value)
    assert len(handles) == 1, "one device scene served every step"
    # what an update cannot express is a new device scene, as before
    fewer = cases.copy(flat, lights=flat.lights[:-1])
    assert_same_frame(render(cfg, fewer, win, renderer=plain), render(cfg, fewer, win, renderer=in_place), "a light less")


# ---- 7. refusals that need a handle ---------------------------------------------------------------------------------------------
def test_refusals_on_a_handle():
    name = "test_scene"
    cfg = CONFIGS["direct"]()
    flat = SCENES[name]()
    lib = _lib.load()
    ds = DeviceScene(flat, 0)
    win = WINDOWS[name]
    before = render(cfg, ds, win)
    turned = cases.animation(name, flat)[2][1]
    groups = _abi.scene_delta_groups(flat, turned)

    def code(change=lambda d: None, new=turned, g=groups):
        d, keep = _abi.make_scene_delta(new, g)
        change(d)
        rc = lib.rt_scene_update(ds.handle, C.byref(d), None)
        return rc, lib.rt_last_error().decode()

    # a progressive render owns the scene
    p, keep = _abi.make_params(cfg)
    buf = np.zeros(cfg.width * cfg.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 64, C.byref(h)))
    rc, msg = code()
    _lib.check(lib.rt_render_end(h, None))
    assert rc == _abi.RT_ERR_INVALID_ARG and "progressive" in msg
    # a triangle range beyond the scene
    rc, msg = code(lambda d: setattr(d, "tri_first", flat.n_triangles - 1))
    assert rc == _abi.RT_ERR_INVALID_ARG and "tri_first" in msg
    # the transmissive class of a material some triangle uses
    used = int(flat.tri_material[0])
    m = flat.materials.copy()
    transmissive = m[used, 8] != 0 and not abs(m[used, 6]) <= 1.1920929e-7
    m[used, 6], m[used, 8] = (0.0, 1.0) if transmissive else (0.5, 1.0)
    rc, msg = code(new=cases.copy(flat, materials=m), g=dict(spheres=False, triangles=None, materials=True, lights=False))
    assert rc == _abi.RT_ERR_INVALID_ARG and "materials" in msg and "transmissive" in msg
    assert lib.rt_scene_update(None, None, None) == _abi.RT_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        ds.update(cases.copy(flat, lights=flat.lights[:-1]))
    with pytest.raises(ValueError):
        ds.update(cases.copy(flat, tri_material=np.roll(flat.tri_material, 1)))
    assert assert_same_frame(before, render(cfg, ds, win), "a refused update changes nothing")
    ds.close()
