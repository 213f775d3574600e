"""Part poses and the SAH report on the GPU (rt_pose*, csrc/rt_pose.hip; rt_scene_bvh_quality, csrc/rt_sah.hip).
The kernel gives the words of its host model (rt_pose_model); a posed handle renders and answers queries exactly as a
handle CREATED from the model's posed description and as one that took rt_scene_update with the model's arrays; the SAH
sums of the device are those of the host model (rt_sah_packed of rt_refit_packed), integer for integer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_cases as P
import scene_update_cases as cases
from test_bvh_quality_host import probe, sah_packed, sah_value  # noqa: F401  (probe: the host-only fixture)
from test_scene_update_gpu import CONFIGS, WINDOWS, assert_same_frame, rays_into, render
import test_scene_update_host as T
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Rotor3, Similarity3, Vec3
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DevicePose, DeviceScene

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# torch is imported BEFORE librt_hip.so is loaded (tests/test_scene_update_gpu.py): the tests that hand tensors to the
# library run in a child process of their own
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_pose_gpu as T
T.{name}()
print("CHILD-OK")
"""


def _run_child(name):
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=HERE, name=name)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 1. kernel against model ------------------------------------------------------------------------------------------------------
def seeded_rest(nt, ns, seed):
    r = np.random.default_rng(seed)
    f = lambda *shape: r.uniform(-2, 2, shape).astype(F32)  # noqa: E731
    return dict(v1=f(nt, 3), v2=f(nt, 3), v3=f(nt, 3), normal=f(nt, 3), centre=f(ns, 3), radius=r.uniform(0.05, 1.5, ns).astype(F32))


def kernel_cases():
    """(label, rest, parts, rows, nan_ok): covering ranges on either side of the 256-thread workgroup, with sphere counts 1, 3
    and 1100 behind them (so spheres start inside a workgroup, at its first thread, and fill several); the three-part
    layout with its gap in a covering range that starts at 1; the 4096 edge values"""
    out = []
    for nt, ns in ((1, 1), (255, 3), (256, 1100), (257, 0), (0, 3)):
        rest = seeded_rest(nt + 2, ns, 100 + nt)  # (two triangles beyond the range: never read, never written)
        parts = [(1, nt, 0, ns)] if nt else [(0, 0, 0, ns)]
        out.append((f"{nt} triangles, {ns} spheres", rest, parts, P.rows_for(parts, "turn"), False))
    rest = seeded_rest(700, 5, 7)
    parts = P.layouts(700, 5)["three_parts"] + [(0, 0, 1, 3)]
    out.append(("three parts with a gap", rest, parts, P.rows_for(parts, "turn"), False))
    rest, parts, rows = P.edge_case()
    out.append(("edge values", rest, parts, rows, True))
    return out


def test_kernel_equals_the_model_word_for_word():
    _run_child("kernel_equals_the_model_word_for_word")


def kernel_equals_the_model_word_for_word():
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for label, rest, parts, rows, nan_ok in kernel_cases():
        d, keep = P.desc_of(rest, parts)
        h = C.c_void_p()
        _lib.check(lib.rt_pose_create(C.byref(d), 0, C.byref(h)))
        out = P.empty_outputs(rest, parts)
        first, count = C.c_uint32(99), C.c_uint32(99)

        def read():
            _lib.check(lib.rt_pose_read(h, *[out[k].ctypes.data for k in P.TRI_OUT], C.byref(first), C.byref(count),
                                        *[out[k].ctypes.data for k in P.SPH_OUT]))

        read()  # before any kernel: the rest pose, restated
        lo, hi, _ = P.covering(parts)
        assert (first.value, count.value) == (lo, hi - lo), label
        P.assert_same_words(out, P.restated(rest, parts), nan_ok=nan_ok, what=f"{label}: before the first kernel")
        t = torch.from_numpy(np.ascontiguousarray(rows, F32)).to(dev)
        _lib.check(lib.rt_pose_geometry_device(h, C.c_void_p(t.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        read()  # (waits for the kernel)
        P.assert_same_words(out, P.model(rest, parts, rows), nan_ok=nan_ok, what=label)
        P.assert_same_words(out, P.expected(rest, parts, rows), nan_ok=nan_ok, what=label + " (numpy)")
        lib.rt_pose_destroy(h)
        print(f"{label}: {hi - lo} triangles and {out['sphere_r_sq'].shape[0]} spheres equal the model")


# ---- 2. one handle, four steps ------------------------------------------------------------------------------------------------------
def about(centre, rotor, scale, shift=(0.0, 0.0, 0.0)):
    """the similarity that turns by `rotor` and scales by `scale` about `centre`, then shifts"""
    c = Vec3(*centre)
    t = c - rotor.rotate_vec(c) * F32(scale) + Vec3(*shift)
    return Similarity3(t, rotor, scale)


def posed_scene(name):
    """-> (flat0, rest, parts, steps).  flat0: the scene with its geometry restated by the model under the identity, so that
    the rest pose is EXACT for it (e1 = v2 - v1, r_sq = r r).  parts: the scene's mesh, and its last sphere when it has
    spheres.  steps: [(label, transforms)]: turn, turn further, scale down, back to rest."""
    flat = P.SCENES[name]()
    rest = P.rest_of(flat)
    nt, ns = flat.n_triangles, flat.n_spheres
    whole = [(0, nt, 0, ns)] if ns else [(0, nt, 0, 0)]
    g = P.model(rest, whole, _abi.transform_rows([Similarity3.identity()]))
    changed = {k: g[k] for k in P.TRI_OUT}
    if ns:
        changed.update({k: g[k] for k in P.SPH_OUT})
    flat0 = cases.copy(flat, **changed)
    first, count = cases.mesh_range(name, flat)
    parts = [(first, count, 0, 0)] + ([(0, 0, ns - 1, 1)] if ns else [])
    s = slice(first, first + count)
    c = np.concatenate([rest["v1"][s], rest["v2"][s], rest["v3"][s]]).astype(np.float64).mean(0)
    d = cases.diagonal(flat)
    mesh = [about(c, Rotor3.from_euler_angles(0.0, 0.0, 0.2), 1.0, (0.01 * d, -0.005 * d, 0.0)),
            about(c, Rotor3.from_euler_angles(0.1, -0.05, 0.45), 1.0, (0.01 * d, -0.005 * d, 0.0)),
            about(c, Rotor3.from_euler_angles(0.1, -0.05, 0.45), 0.8), Similarity3.identity()]
    if ns:
        cs = rest["centre"][ns - 1]
        ball = [about(cs, Rotor3.identity(), 1.0, (0.02 * d, 0.0, 0.0)), about(cs, Rotor3.identity(), 1.25, (0.02 * d, 0.01 * d, 0.0)),
                about(cs, Rotor3.from_euler_angles(0.3, 0.0, 0.0), 0.7), Similarity3.identity()]
    labels = ("turn", "turn further", "scale down", "back to rest")
    steps = [(labels[k], _abi.transform_rows([mesh[k]] + ([ball[k]] if ns else []))) for k in range(4)]
    return flat0, rest, parts, steps


def posed_flat(flat0, rest, parts, rows):
    """the model's posed description of the whole scene"""
    g = P.model(rest, parts, rows)
    lo, hi, has_spheres = P.covering(parts)
    changed = {}
    for k in P.TRI_OUT:
        a = np.array(getattr(flat0, k), copy=True)
        a[lo:hi] = g[k]
        changed[k] = a
    if has_spheres:
        changed.update({k: g[k] for k in P.SPH_OUT})
    return cases.copy(flat0, **changed)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def new_pose(ds, rest, parts):
    return DevicePose(ds, parts, rest_v2=rest["v2"], rest_v3=rest["v3"], rest_radius=rest["radius"])


@pytest.mark.parametrize("name,config", [("semesterbild", "soft"), ("test_scene", "realistic")])
def test_four_steps_on_one_handle_equal_fresh_and_updated_handles(name, config):
    cfg, win = CONFIGS[config](), WINDOWS[name]
    flat0, rest, parts, steps = posed_scene(name)
    ds, upd = DeviceScene(flat0, 0), DeviceScene(flat0, 0)
    pose = new_pose(ds, rest, parts)
    first = render(cfg, ds, win)
    o, d = rays_into(flat0, 1021, 9)
    changed = []
    for label, rows in steps:
        what = f"{name} / {config} / {label}"
        want = posed_flat(flat0, rest, parts, rows)
        info = pose.apply(rows, info=True)
        assert info["device_ms"] > 0 and info["nodes_refitted"] == ds.bvh_info()["n_nodes"] and info["slots_rewritten"] == P.covering(parts)[1] - P.covering(parts)[0]
        for k in P.TRI_OUT + P.SPH_OUT:
            assert np.array_equal(bits(getattr(ds.flat, k)), bits(getattr(want, k))), f"{what}: scene.flat.{k} follows"
        got = render(cfg, ds, win)
        fresh_ds = DeviceScene(want, 0)
        assert_same_frame(got, render(cfg, fresh_ds, win), what + " vs a handle created from the model's description")
        upd.update(want)
        assert_same_frame(got, render(cfg, upd, win), what + " vs a handle updated with the model's arrays")
        hits = ds.cast_rays(o, d)
        for a, b, c, field in zip(hits, fresh_ds.cast_rays(o, d), upd.cast_rays(o, d), hits._fields):
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)), f"{what}: cast_rays.{field}"
        fresh_ds.close()
        changed.append(not np.array_equal(got[1]["hit_t"].view(np.uint32), first[1]["hit_t"].view(np.uint32)))
        print(f"{what}: apply {info['total_ms']:.3f} ms wall, {info['device_ms']:.3f} ms device; frame differs from the rest frame: {changed[-1]}")
    assert changed[:3] == [True, True, True], "the window shows what moves"
    assert assert_same_frame(got, first, f"{name} / {config}: back at rest"), "the float planes too"
    pose.close(), ds.close(), upd.close()


# ---- 3. device form, 4. view frame (children: torch tensors) ------------------------------------------------------------------------
def test_device_form_equals_host_form():
    """a torch tensor of transforms on the device (rt_pose_apply_device) gives the frames of the host form, step by step"""
    _run_child("device_form_equals_host_form")


def device_form_equals_host_form():
    import torch

    name = "test_scene"
    cfg, win = CONFIGS["soft"](), WINDOWS[name]
    flat0, rest, parts, steps = posed_scene(name)
    host, devf = DeviceScene(flat0, 0), DeviceScene(flat0, 0)
    ph, pd = new_pose(host, rest, parts), new_pose(devf, rest, parts)
    dev = torch.device("cuda", 0)
    for label, rows in steps:
        ph.apply(rows)
        info = pd.apply(torch.from_numpy(rows).to(dev), info=True)
        assert info["device_ms"] > 0
        for k in P.TRI_OUT + P.SPH_OUT:
            assert np.array_equal(bits(getattr(devf.flat, k)), bits(getattr(host.flat, k))), "the description it holds follows"
        assert assert_same_frame(render(cfg, devf, win), render(cfg, host, win), f"device form / {label}"), "float planes too"
    with pytest.raises(ValueError):
        pd.apply(torch.zeros((len(parts) + 1, 8), device=dev))
    with pytest.raises(ValueError):
        pd.apply(torch.zeros((len(parts), 8), dtype=torch.float64, device=dev))
    ph.close(), pd.close(), host.close(), devf.close()


def test_view_frame_after_a_device_pose_shows_the_posed_scene():
    """rt_pose_apply_device and rt_render_view_device on one stream: the view's frame is the same view of a fresh handle"""
    _run_child("view_frame_after_a_device_pose")


def view_frame_after_a_device_pose():
    import torch

    import view_cases as vc
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceView

    name = "test_scene"
    flat0, rest, parts, steps = posed_scene(name)
    cfg = RenderConfig.from_features(["realistic"])
    w, h = 37, 29
    smp = vc.sample_tables(_abi.RT_VIEW_PINHOLE)["repeats9"]
    view = DeviceView(0, w, h, smp, camera=vc.pinhole(w, h).view_camera())
    ds = DeviceScene(flat0, 0)
    pose = new_pose(ds, rest, parts)
    dev = torch.device("cuda", 0)
    before = ds.render_view(view, cfg, torch_out=True)
    rows = steps[1][1]
    pose.apply(torch.from_numpy(rows).to(dev))
    after = ds.render_view(view, cfg, torch_out=True)
    torch.cuda.synchronize(dev)
    fresh = DeviceScene(posed_flat(flat0, rest, parts, rows), 0)
    want = fresh.render_view(view, cfg)
    got = {k: getattr(after, k).cpu().numpy() for k in ("rgb", "valid", "id", "t")}
    for k in got:
        assert np.array_equal(bits(got[k]), bits(getattr(want, k))), f"view frame after the pose: {k}"
    assert not np.array_equal(bits(before.t.cpu().numpy()), bits(got["t"])), "the view shows what moved"
    view.close(), pose.close(), ds.close(), fresh.close()


# ---- 5. SAH report ----------------------------------------------------------------------------------------------------------------
def host_sums(probe, flat, then=None):  # noqa: F811
    """rt_sah_packed of the packed scene, after rt_refit_packed to `then` when given"""
    T.pack(probe, 0, flat)
    if then is not None:
        assert T.refit(probe, 0, flat, then) == 0, probe.probe_error()
    return sah_packed(probe, 0)


def check_quality(q, now, created):
    assert (q["inner_q"], q["leaf_q"], q["n_bad"]) == now, (q, now)
    assert q["sah_now"] == sah_value(*now[:2]) and q["sah_created"] == sah_value(*created[:2])


def test_bvh_quality_follows_updates_and_poses(probe):  # noqa: F811
    flat0, rest, parts, steps = posed_scene("semesterbild")
    created = host_sums(probe, flat0)
    ds = DeviceScene(flat0, 0)
    q = ds.bvh_quality()
    check_quality(q, created, created)
    assert q["sah_now"] == q["sah_created"] > 0 and q["device_ms"] > 0
    moved = cases.jitter(flat0, 0.05)
    ds.update(moved)
    q = ds.bvh_quality()
    check_quality(q, host_sums(probe, flat0, moved), created)
    print(f"5 % jitter: sah {q['sah_created']:.4f} -> {q['sah_now']:.4f}, report {q['device_ms']:.3f} ms")
    assert q["sah_now"] > q["sah_created"]
    ds.update(flat0)
    check_quality(ds.bvh_quality(), created, created)
    pose = new_pose(ds, rest, parts)
    rows = steps[2][1]
    pose.apply(rows)
    q = ds.bvh_quality()
    check_quality(q, host_sums(probe, flat0, posed_flat(flat0, rest, parts, rows)), created)
    print(f"posed: sah {q['sah_created']:.4f} -> {q['sah_now']:.4f}")
    pose.close(), ds.close()


# soup(n) (pose_cases.py, seed 40) builds these trees: 1 node; 255, 256 and 257 nodes -- one workgroup less a thread, one
# workgroup exactly, one workgroup and a thread
NODE_COUNTS = {3: 1, 433: 255, 431: 256, 432: 257}


@pytest.mark.parametrize("n", sorted(NODE_COUNTS))
def test_bvh_quality_at_the_workgroup_edge(probe, n):  # noqa: F811
    flat = P.soup(n)
    ds = DeviceScene(flat, 0)
    assert ds.bvh_info()["n_nodes"] == NODE_COUNTS[n], "the builder changed: choose the triangle counts again"
    created = host_sums(probe, flat)
    check_quality(ds.bvh_quality(), created, created)
    moved = cases.jitter(flat, 0.05)
    ds.update(moved)
    check_quality(ds.bvh_quality(), host_sums(probe, flat, moved), created)
    ds.close()


def test_bvh_quality_of_a_scene_without_triangles():
    flat = cases.flat_test_scene().without_triangles().contiguous()
    ds = DeviceScene(flat, 0)
    q = ds.bvh_quality()
    assert q["sah_created"] == 0.0 and q["sah_now"] == 0.0 and (q["inner_q"], q["leaf_q"], q["n_bad"]) == (0, 0, 0)
    ds.close()


# ---- 6. refusals that need a handle -------------------------------------------------------------------------------------------------
def test_apply_refusals():
    lib = _lib.load()
    flat0, rest, parts, steps = posed_scene("test_scene")
    ds = DeviceScene(flat0, 0)
    pose = new_pose(ds, rest, parts)
    cfg, win = CONFIGS["direct"](), WINDOWS["test_scene"]
    before = render(cfg, ds, win)
    bad = _abi.RT_ERR_INVALID_ARG
    rows = steps[0][1]

    def code(scene, p, t):
        rc = lib.rt_pose_apply(scene, p, None if t is None else t.ctypes.data, None)
        return rc, lib.rt_last_error().decode()

    assert code(None, pose.handle, rows) == (bad, "rt_pose_apply: null scene")
    rc, msg = code(ds.handle, None, rows)
    assert rc == bad and "null pose" in msg
    rc, msg = code(ds.handle, pose.handle, None)
    assert rc == bad and "null transforms" in msg
    for k, value in ((0, np.nan), (3, np.inf), (7, -np.inf), (8 + 7, np.nan)):
        r = rows.copy()
        r.reshape(-1)[k] = value
        rc, msg = code(ds.handle, pose.handle, r)
        assert rc == bad and f"transform {k // 8} has a non-finite member" in msg, msg
    # a pose for another scene's counts
    fewer = cases.copy(flat0, sphere_center=flat0.sphere_center[:-1], sphere_r_sq=flat0.sphere_r_sq[:-1], sphere_r_inv=flat0.sphere_r_inv[:-1],
                       sphere_material=flat0.sphere_material[:-1])
    other = DeviceScene(fewer, 0)
    rc, msg = code(other.handle, pose.handle, rows)
    assert rc == bad and "the pose is for" in msg and "the scene has" in msg
    rc = lib.rt_pose_apply_device(other.handle, pose.handle, C.c_void_p(256), None, None)  # (refused before the pointer is used)
    assert rc == bad and "the pose is for" in lib.rt_last_error().decode()
    # what rt_scene_update_device refuses: a split-clipped tree, a progressive render
    clipped = DeviceScene(flat0, 0, bvh=dict(split_depth=8, split_gain=0.99))
    if clipped.bvh_info()["n_references"] > flat0.n_triangles:
        rc, msg = code(clipped.handle, pose.handle, rows)
        assert rc == _abi.RT_ERR_UNSUPPORTED and "split clipping" in msg
    p, keep = _abi.make_params(cfg)
    buf = np.zeros(cfg.width * cfg.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 64, C.byref(h)))
    rc, msg = code(ds.handle, pose.handle, rows)
    _lib.check(lib.rt_render_end(h, None))
    assert rc == bad and "progressive" in msg
    assert assert_same_frame(before, render(cfg, ds, win), "a refused apply changes nothing")
    g = pose.geometry()
    assert np.array_equal(g["tri_v1"], flat0.tri_v1[g["tri_first"]:g["tri_first"] + g["tri_count"]]), "... not the pose's arrays either"
    with pytest.raises(ValueError):
        pose.apply(rows[:1])
    pose.close(), ds.close(), other.close(), clipped.close()


# ---- 7. the C example -----------------------------------------------------------------------------------------------------------------
def test_c_pose_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_pose_example"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_pose_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step 3 restores the checksum of step 1" in out.stdout and "sah" in out.stdout
