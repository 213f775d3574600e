"""Device-side BVH rebuilds on the GPU (rt_scene_rebuild, csrc/rt_rebuild.cpp): a handle whose tree has been rebuilt renders
and answers queries as a handle freshly created from the same geometry.  The tree only prunes work, so hit ids and hit
distances are the same bits; colours are held to the project's bar RGB_TOL, because the shadow products of a pixel may be
summed in another leaf-slot order (whether they came out bit-equal anyway is printed, and recorded in profiles/rebuild.md).
What the handle reports about its tree is held to the host model (tests/test_rebuild_host.py), the SAH sums bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_query_cases as fq
import scene_update_cases as cases
from test_pose_gpu import new_pose, posed_flat, posed_scene
from test_rebuild_host import info_of, probe, rebuilt, sah_of  # noqa: F401  (probe: the host-only fixture)
from test_scene_update_gpu import CONFIGS, RGB_TOL, SCENES, WINDOWS, assert_same_frame, render
from test_scene_update_host import pack, refit
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EVERYTHING = _abi.RT_UPDATE_INVALIDATES_RECEIVER_TABLES | _abi.RT_UPDATE_INVALIDATES_TILE_COSTS | _abi.RT_UPDATE_INVALIDATES_QUEUE_SIZES
RAYS = {"test_scene": "test_scene", "semesterbild": "text_lowres"}  # the ray sets of f64_query_cases


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def deformed(name, flat):
    """turn + jitter, as the update tests apply them"""
    d = cases.diagonal(flat)
    return cases.jitter(cases.turn_mesh(flat, cases.mesh_range(name, flat), 20.0, (0.01 * d, -0.005 * d, 0.0)), 0.05)


def assert_equivalent_frame(a, b, what):
    """ids and t planes bit-identical, rgb within the project's bar, equal ray counters; -> whether the rgb planes are bit-equal too"""
    assert np.array_equal(a[1]["hit_id"], b[1]["hit_id"]), f"{what}: hit ids differ"
    assert np.array_equal(a[1]["hit_t"].view(np.uint32), b[1]["hit_t"].view(np.uint32)), f"{what}: hit t differs"
    d = float(np.abs(a[1]["rgb"] - b[1]["rgb"]).max())
    equal = np.array_equal(a[1]["rgb"].view(np.uint32), b[1]["rgb"].view(np.uint32))
    print(f"{what}: max |dRGB| = {d:.3e}; float rgb bit-equal: {equal}; packed pixels equal: {np.array_equal(a[0], b[0])}")
    assert d <= RGB_TOL, f"{what}: |dRGB| {d:.3e} > {RGB_TOL}"
    for sh in (24, 16, 8, 0):
        assert np.abs(((a[0] >> sh) & 0xFF).astype(np.int32) - ((b[0] >> sh) & 0xFF).astype(np.int32)).max() <= 1, what
    for k in ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "pixels_written"):
        assert a[2][k] == b[2][k], (what, k, a[2][k], b[2][k])
    return equal


def assert_equivalent_queries(ds, fresh, name, what):
    o, d, kind, max_d = fq.rays(RAYS[name])
    assert len(o) == 1021
    hits, want = ds.cast_rays(o, d), fresh.cast_rays(o, d)
    for a, b, field in zip(hits, want, hits._fields):
        assert np.array_equal(bits(a), bits(b)), f"{what}: cast_rays.{field}"
    assert (hits.id >= 0).sum() > 200, "the rays meet the scene"
    occ, want = ds.any_intersection(o, d, max_d), fresh.any_intersection(o, d, max_d)
    assert np.array_equal(occ.has_intersection, want.has_intersection) and np.array_equal(occ.completely_occluded, want.completely_occluded), what
    assert np.abs(occ.combined_opacity - want.combined_opacity).max() <= RGB_TOL, f"{what}: any_intersection.combined_opacity"
    part = ~occ.completely_occluded  # (the filter is unspecified where completely occluded)
    assert np.abs(occ.color_filter[part] - want.color_filter[part]).max(initial=0.0) <= RGB_TOL, f"{what}: any_intersection.color_filter"
    cfg = CONFIGS["realistic"]()
    rad, want = ds.trace_rays(o, d, cfg), fresh.trace_rays(o, d, cfg)
    assert np.array_equal(rad.id, want.id) and np.array_equal(bits(rad.t), bits(want.t)) and np.array_equal(rad.valid, want.valid), f"{what}: trace_rays ids / t"
    assert np.abs(rad.rgb - want.rgb).max() <= RGB_TOL, f"{what}: trace_rays.rgb"
    equal = np.array_equal(bits(rad.rgb), bits(want.rgb))
    print(f"{what}: trace_rays max |dRGB| = {float(np.abs(rad.rgb - want.rgb).max()):.3e}; bit-equal: {equal}")


# ---- 1. a rebuilt handle against a fresh one, and against the host model ---------------------------------------------------------
@pytest.mark.parametrize("case", ["fresh", "deformed"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_rebuilt_handle_answers_as_a_fresh_one(probe, name, case):  # noqa: F811
    flat = SCENES[name]()
    now = deformed(name, flat) if case == "deformed" else flat
    what = f"{name} / {case}"
    ds = DeviceScene(flat, 0)
    created = ds.bvh_quality()
    if now is not flat:
        ds.update(now)
    refitted = ds.bvh_quality()
    info = ds.rebuild(info=True)
    fresh = DeviceScene(now, 0)
    # the host model of the same history
    pack(probe, 0, flat)
    if now is not flat:
        assert refit(probe, 0, flat, now) == 0, probe.probe_error()
    rebuilt(probe, now)
    want = info_of(probe, 0)
    sums, sah, bad = sah_of(probe, 0)
    assert info["tables_invalidated"] == EVERYTHING and info["device_ms"] > 0 and info["total_ms"] >= info["device_ms"] * 0.5
    assert {k: info[k] for k in ("n_nodes", "n_leaves", "max_depth", "max_leaf_size")} == {k: want[k] for k in ("n_nodes", "n_leaves", "max_depth", "max_leaf_size")}
    bi = ds.bvh_info()
    assert {k: bi[k] for k in ("n_nodes", "n_leaves", "max_depth", "max_leaf_size", "n_references", "bytes_nodes", "bytes_triangles")} == \
        {k: want[k] for k in ("n_nodes", "n_leaves", "max_depth", "max_leaf_size", "n_references", "bytes_nodes", "bytes_triangles")}
    assert ds.memory_info()["bytes_bvh"] == want["bytes_bvh"]
    q = ds.bvh_quality()
    assert (q["inner_q"], q["leaf_q"], q["n_bad"]) == (sums[0], sums[1], bad), "the integer SAH sums, bit for bit"
    assert q["sah_now"] == sah and q["sah_created"] == created["sah_created"], "sah_created stays the value of creation"
    print(f"{what}: rebuild {info['total_ms']:.3f} ms wall, {info['device_ms']:.3f} ms device; {info['n_nodes']} nodes, depth {info['max_depth']}; "
          f"SAH created {created['sah_created']:.2f}, refitted {refitted['sah_now']:.2f}, rebuilt {q['sah_now']:.2f}")
    assert_equivalent_queries(ds, fresh, name, what)
    equal = [assert_equivalent_frame(render(CONFIGS[c](), ds, WINDOWS[name]), render(CONFIGS[c](), fresh, WINDOWS[name]), f"{what} / {c}") for c in sorted(CONFIGS)]
    print(f"{what}: float rgb planes bit-equal to a fresh handle's in {sum(equal)} of {len(equal)} configurations")
    ds.close(), fresh.close()


# ---- 2. soft-shadow tables ----------------------------------------------------------------------------------------------------------
def test_soft_shadow_frame_after_a_rebuild_reruns_the_flags_kernel():
    name = "semesterbild"
    cfg, win = CONFIGS["soft"](), (200, 150, 320, 240)
    flat = SCENES[name]()
    ds = DeviceScene(flat, 0, budget=2 << 30)  # (opted in: the per-cell candidate lists fit -- they hold leaf slots)
    render(cfg, ds, win)
    mi = ds.memory_info()
    assert mi["n_receiver_cells"] > 0 and mi["cell_lists_built"] == 1 and mi["bytes_cell_lists"] > 0
    ds.rebuild()
    mid = ds.memory_info()
    assert mid["n_receiver_cells"] == mi["n_receiver_cells"] and mid["cell_lists_built"] == 0
    got = render(cfg, ds, win)
    assert got[2]["setup_ms"] > 0.0, "the flags were rebuilt by this frame"
    after = ds.memory_info()
    assert after["cell_lists_built"] == 1 and after["bytes_cell_lists"] == mi["bytes_cell_lists"] and after["bytes_flags"] == mi["bytes_flags"]
    fresh = DeviceScene(flat, 0, budget=2 << 30)
    assert_equivalent_frame(got, render(cfg, fresh, win), "soft shadows, lists on, after a rebuild")
    ds.close(), fresh.close()


# ---- 3. updates and poses after a rebuild -------------------------------------------------------------------------------------------
def test_update_and_pose_after_a_rebuild_still_match_fresh_handles():
    name = "semesterbild"
    cfg, win = CONFIGS["soft"](), WINDOWS[name]
    flat0, rest, parts, steps = posed_scene(name)
    ds = DeviceScene(flat0, 0)
    pose = new_pose(ds, rest, parts)
    ds.rebuild()
    moved = cases.jitter(flat0, 0.05)
    info = ds.update(moved, info=True)
    assert info["nodes_refitted"] == ds.bvh_info()["n_nodes"] and info["slots_rewritten"] == flat0.n_triangles
    fresh = DeviceScene(moved, 0)
    assert_equivalent_frame(render(cfg, ds, win), render(cfg, fresh, win), "update after a rebuild")
    assert_equivalent_queries(ds, fresh, name, "update after a rebuild")
    fresh.close()
    ds.update(flat0)
    rows = steps[1][1]
    pose.apply(rows)
    want = posed_flat(flat0, rest, parts, rows)
    fresh = DeviceScene(want, 0)
    assert_equivalent_frame(render(cfg, ds, win), render(cfg, fresh, win), "pose after a rebuild")
    ds.rebuild()
    assert_equivalent_frame(render(cfg, ds, win), render(cfg, fresh, win), "a second rebuild, of the posed scene")
    pose.close(), ds.close(), fresh.close()


# ---- 4. frames in flight (a child: torch streams; torch is imported BEFORE librt_hip.so is loaded) -----------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_rebuild_gpu as T
T.{name}()
print("CHILD-OK")
"""


def test_rebuild_waits_for_the_frames_in_flight():
    """two frames enqueued on two streams, then rt_scene_rebuild without a synchronisation of the caller's: both frames were
    rendered from the old blob before it was freed, the next one from the new"""
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=HERE, name="rebuild_waits_for_the_frames_in_flight")],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def rebuild_waits_for_the_frames_in_flight():
    import torch

    cfg = CONFIGS["soft"]()
    flat = SCENES["semesterbild"]()
    frame = render(cfg, flat)[0]
    lib = _lib.load()
    ds = DeviceScene(flat, 0)
    p, keep = _abi.make_params(cfg)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    fbs = [torch.zeros(cfg.width * cfg.height, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    for k in range(2):
        _lib.check(lib.rt_render_device(ds.handle, C.byref(p), C.c_void_p(fbs[k].data_ptr()), None, C.c_void_p(streams[k].cuda_stream)))
    _lib.check(lib.rt_scene_rebuild(ds.handle, None))
    _lib.check(lib.rt_render_device(ds.handle, C.byref(p), C.c_void_p(fbs[2].data_ptr()), None, C.c_void_p(streams[0].cuda_stream)))
    torch.cuda.synchronize(dev)
    got = [fb.cpu().numpy().view(np.uint32) for fb in fbs]
    assert np.array_equal(got[0], frame) and np.array_equal(got[1], frame), "the frames in flight were rendered from the old blob"
    assert np.array_equal(got[2] != 0, frame != 0)
    for sh in (24, 16, 8, 0):
        assert np.abs(((got[2] >> sh) & 0xFF).astype(np.int32) - ((frame >> sh) & 0xFF).astype(np.int32)).max() <= 1, "the next frame shows the same scene"
    # the device form on a stream of the caller's
    info = _abi.rt_rebuild_info()
    _lib.check(lib.rt_scene_rebuild_device(ds.handle, C.c_void_p(streams[1].cuda_stream), C.byref(info)))
    assert info.n_nodes == ds.bvh_info()["n_nodes"] and info.device_ms > 0
    ds.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    name = "test_scene"
    cfg, win = CONFIGS["direct"](), WINDOWS[name]
    flat = SCENES[name]()
    lib = _lib.load()

    def code(handle):
        rc = lib.rt_scene_rebuild(handle, None)
        return rc, lib.rt_last_error().decode()

    rc, msg = code(None)
    assert rc == _abi.RT_ERR_INVALID_ARG and "null scene" in msg
    assert lib.rt_scene_rebuild_device(None, None, None) == _abi.RT_ERR_INVALID_ARG
    ds = DeviceScene(flat, 0)
    before, info_before = render(cfg, ds, win), ds.bvh_info()
    p, keep = _abi.make_params(cfg)
    buf = np.zeros(cfg.width * cfg.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 64, C.byref(h)))
    rc, msg = code(ds.handle)
    _lib.check(lib.rt_render_end(h, None))
    assert rc == _abi.RT_ERR_INVALID_ARG and "progressive" in msg
    assert ds.bvh_info() == info_before and assert_same_frame(before, render(cfg, ds, win), "refused: progressive render"), "the float planes too"
    ds.close()
    empty = DeviceScene(flat.without_triangles().contiguous(), 0)
    before = render(cfg, empty, win)
    rc, msg = code(empty.handle)
    assert rc == _abi.RT_ERR_INVALID_ARG and "nothing to rebuild" in msg
    assert assert_same_frame(before, render(cfg, empty, win), "refused: no triangles")
    empty.close()
    clipped = DeviceScene(flat, 0, bvh=dict(split_depth=8, split_gain=0.99))
    assert clipped.bvh_info()["n_references"] > flat.n_triangles, "the case is split-clipped"
    before, info_before = render(cfg, clipped, win), clipped.bvh_info()
    rc, msg = code(clipped.handle)
    assert rc == _abi.RT_ERR_UNSUPPORTED and "split clipping" in msg
    with pytest.raises(_lib.RtError):
        clipped.rebuild()
    assert clipped.bvh_info() == info_before and assert_same_frame(before, render(cfg, clipped, win), "refused: split clipping"), "the float planes too"
    clipped.close()


# ---- 6. the C example -------------------------------------------------------------------------------------------------------------------
def test_c_rebuild_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_rebuild_example"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_rebuild_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rebuilt" in out.stdout and "checksum" in out.stdout and "hit ids equal" in out.stdout
