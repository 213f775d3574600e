"""Skinned meshes on the GPU (rt_skin*, csrc/rt_skin.hip).  The kernels give the words of their host model (rt_skin_model)
and of the numpy restatement; a skinned handle renders and answers queries exactly as a handle CREATED from the model's
description and as one that took rt_scene_update with the model's arrays; the SAH report after a bend is the host model's,
integer for integer, and a rebuild after it answers as a fresh handle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import skin_cases as S
from test_bvh_quality_host import probe  # noqa: F401  (the host-only fixture)
from test_pose_gpu import check_quality, host_sums
from test_scene_update_gpu import CONFIGS, WINDOWS, assert_same_frame, rays_into, render
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import IndexedMesh
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, DeviceSkin

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = {"semesterbild": S.semesterbild_skin, "strip": S.strip_scene}
# the bend of the SAH test, chosen on the CPU with the host model (rt_refit_packed + rt_sah_packed of semesterbild_skin):
# the refitted tree costs more than the tree of creation from a few degrees on; 60 degrees is far inside
LARGE_BEND = 60.0

# torch is imported BEFORE librt_hip.so is loaded (tests/test_scene_update_gpu.py): the tests that hand tensors to the
# library run in a child process of their own
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_skin_gpu as T
T.{name}()
print("CHILD-OK")
"""


def _run_child(name):
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=HERE, name=name)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def new_skin(ds, mesh):
    return DeviceSkin(ds, IndexedMesh(mesh["position"], mesh["normal"], mesh["indices"]), mesh["bone"], mesh["weight"], tri_first=mesh["tri_first"],
                      n_bones=mesh["n_bones"])


# ---- 6. kernels against model -------------------------------------------------------------------------------------------------------
def kernel_cases():
    """(label, mesh, bones, nan_ok): the seeded sizes on either side of the 256-thread workgroup in both normal modes, and the
    4096 edge values in both"""
    out = [(label, mesh, bones, len(mesh["position"]) == 1 and mesh["normal"] is None) for label, mesh, bones in S.seeded_cases()]
    for normals in (True, False):
        mesh, bones = S.edge_case(normals)
        out.append((f"edge values, {'vertex' if normals else 'face'} normals", mesh, bones, True))
    return out


def test_kernels_equal_the_model_word_for_word():
    _run_child("kernels_equal_the_model_word_for_word")


def kernels_equal_the_model_word_for_word():
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for label, mesh, bones, nan_ok in kernel_cases():
        d, keep = S.desc_of(mesh)
        h = C.c_void_p()
        _lib.check(lib.rt_skin_create(C.byref(d), 0, C.byref(h)))
        out = S.empty_outputs(mesh)
        _lib.check(lib.rt_skin_read(h, *S.pointers(out)))  # before any kernel: the rest mesh through the triangle formula
        S.assert_same_words(out, S.restated(mesh), nan_ok=nan_ok, what=f"{label}: before the first kernel")
        t = torch.from_numpy(np.ascontiguousarray(bones, F32)).to(dev)
        _lib.check(lib.rt_skin_geometry_device(h, C.c_void_p(t.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        _lib.check(lib.rt_skin_read(h, *S.pointers(out)))  # (waits for the kernels)
        S.assert_same_words(out, S.model(mesh, bones), nan_ok=nan_ok, what=label)
        S.assert_same_words(out, S.expected(mesh, bones), nan_ok=nan_ok, what=label + " (numpy)")
        lib.rt_skin_destroy(h)
        print(f"{label}: {len(mesh['position'])} vertices and {len(mesh['indices'])} triangles equal the model")


# ---- 7. one handle, four steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", [("semesterbild", "soft"), ("strip", "realistic")])
def test_four_steps_on_one_handle_equal_fresh_and_updated_handles(name, config):
    cfg, win = CONFIGS[config](), WINDOWS.get(name)
    flat0, mesh = SCENES[name]()
    ds, upd = DeviceScene(flat0, 0), DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    first = render(cfg, ds, win)
    o, d = rays_into(flat0, 1021, 9)
    changed = []
    for label, bones in S.four_steps(mesh):
        what = f"{name} / {config} / {label}"
        want = S.with_mesh(flat0, mesh, bones)
        info = skin.apply(bones, info=True)
        assert info["device_ms"] > 0 and info["nodes_refitted"] == ds.bvh_info()["n_nodes"] and info["slots_rewritten"] == len(mesh["indices"])
        for k in S.TRI_OUT:
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
    assert changed[:3] == [True, True, True], "the frame shows what bends"
    assert assert_same_frame(got, first, f"{name} / {config}: back at rest"), "the float planes too"
    skin.close(), ds.close(), upd.close()


# ---- 8. device form, 9. view frame (children: torch tensors) ----------------------------------------------------------------------------
def test_device_form_equals_host_form():
    """a torch tensor of bones on the device (rt_skin_apply_device) gives the frames of the host form, step by step"""
    _run_child("device_form_equals_host_form")


def device_form_equals_host_form():
    import torch

    cfg = CONFIGS["direct"]()
    flat0, mesh = S.strip_scene(normals=False)
    host, devf = DeviceScene(flat0, 0), DeviceScene(flat0, 0)
    sh, sd = new_skin(host, mesh), new_skin(devf, mesh)
    dev = torch.device("cuda", 0)
    for label, bones in S.four_steps(mesh):
        sh.apply(bones)
        info = sd.apply(torch.from_numpy(bones).to(dev), info=True)
        assert info["device_ms"] > 0 and info["slots_rewritten"] == len(mesh["indices"])
        for k in S.TRI_OUT:
            assert np.array_equal(bits(getattr(devf.flat, k)), bits(getattr(host.flat, k))), "the description it holds follows"
        S.assert_same_words(sd.geometry(), sh.geometry(), what=f"device form / {label}")
        assert assert_same_frame(render(cfg, devf), render(cfg, host), f"device form / {label}"), "float planes too"
    with pytest.raises(ValueError):
        sd.apply(torch.zeros((3, 8), device=dev))
    with pytest.raises(ValueError):
        sd.apply(torch.zeros((2, 8), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        sd.apply(torch.zeros((2, 8)))  # (on the host)
    with pytest.raises(ValueError):
        sd.apply(np.zeros((2, 7), F32))
    with pytest.raises(ValueError):
        sd.apply(np.zeros((2, 8), np.float64))
    sh.close(), sd.close(), host.close(), devf.close()


def test_view_frame_after_a_device_skin_shows_the_bent_mesh():
    """rt_skin_apply_device and rt_render_view_device on one stream: the view's frame is the same view of a fresh handle"""
    _run_child("view_frame_after_a_device_skin")


def view_frame_after_a_device_skin():
    import torch

    import view_cases as vc
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceView

    flat0, mesh = S.strip_scene()
    cfg = RenderConfig.from_features(["realistic"])
    w, h = 37, 29
    smp = vc.sample_tables(_abi.RT_VIEW_PINHOLE)["repeats9"]
    view = DeviceView(0, w, h, smp, camera=vc.pinhole(w, h).view_camera())
    ds = DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    dev = torch.device("cuda", 0)
    before = ds.render_view(view, cfg, torch_out=True)
    bones = S.four_steps(mesh)[1][1]
    skin.apply(torch.from_numpy(bones).to(dev))
    after = ds.render_view(view, cfg, torch_out=True)
    torch.cuda.synchronize(dev)
    fresh = DeviceScene(S.with_mesh(flat0, mesh, bones), 0)
    want = fresh.render_view(view, cfg)
    got = {k: getattr(after, k).cpu().numpy() for k in ("rgb", "valid", "id", "t")}
    for k in got:
        assert np.array_equal(bits(got[k]), bits(getattr(want, k))), f"view frame after the skin: {k}"
    assert not np.array_equal(bits(before.t.cpu().numpy()), bits(got["t"])), "the view shows what bent"
    view.close(), skin.close(), ds.close(), fresh.close()


# ---- 10. SAH report and rebuild after a bend ----------------------------------------------------------------------------------------------
def test_bvh_quality_after_a_bend_and_a_rebuild_after_it(probe):  # noqa: F811
    flat0, mesh = S.semesterbild_skin()
    created = host_sums(probe, flat0)
    ds = DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    check_quality(ds.bvh_quality(), created, created)
    for degrees in (5.0, LARGE_BEND):
        bones = S.bend(mesh, degrees)
        want = S.with_mesh(flat0, mesh, bones)
        skin.apply(bones)
        q = ds.bvh_quality()
        check_quality(q, host_sums(probe, flat0, want), created)
        print(f"bent by {degrees} degrees: sah {q['sah_created']:.4f} -> {q['sah_now']:.4f}")
    assert q["sah_now"] > q["sah_created"], "a large bend loosens the refitted tree"
    ds.rebuild()
    fresh = DeviceScene(want, 0)
    cfg, win = CONFIGS["direct"](), WINDOWS["semesterbild"]
    a, b = render(cfg, ds, win), render(cfg, fresh, win)
    assert np.array_equal(a[1]["hit_id"], b[1]["hit_id"]) and np.array_equal(a[1]["hit_t"].view(np.uint32), b[1]["hit_t"].view(np.uint32))
    o, d = rays_into(want, 1021, 9)
    hits, ref = ds.cast_rays(o, d), fresh.cast_rays(o, d)
    assert np.array_equal(hits.id, ref.id) and np.array_equal(bits(hits.t), bits(ref.t)), "ids and t of a rebuilt handle are a fresh handle's"
    assert (hits.id >= 0).sum() > 200, "the rays meet the scene"
    # the skin speaks in canonical indices: it goes on working on the rebuilt tree
    bones = S.bend(mesh, 20.0)
    skin.apply(bones)
    again = DeviceScene(S.with_mesh(flat0, mesh, bones), 0)
    a, b = render(cfg, ds, win), render(cfg, again, win)
    assert np.array_equal(a[1]["hit_id"], b[1]["hit_id"]) and np.array_equal(a[1]["hit_t"].view(np.uint32), b[1]["hit_t"].view(np.uint32))
    skin.close(), ds.close(), fresh.close(), again.close()


# ---- 11. refusals that need a handle --------------------------------------------------------------------------------------------------------
def test_apply_refusals():
    lib = _lib.load()
    flat0, mesh = S.strip_scene()
    ds = DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    cfg = CONFIGS["direct"]()
    before, rest = render(cfg, ds), skin.geometry()
    bad = _abi.RT_ERR_INVALID_ARG
    bones = S.four_steps(mesh)[0][1]

    def code(scene, s, t):
        rc = lib.rt_skin_apply(scene, s, None if t is None else t.ctypes.data, None)
        return rc, lib.rt_last_error().decode()

    assert code(None, skin.handle, bones) == (bad, "rt_skin_apply: null scene")
    rc, msg = code(ds.handle, None, bones)
    assert rc == bad and "null skin" in msg
    rc, msg = code(ds.handle, skin.handle, None)
    assert rc == bad and "null bones" in msg
    for k, value in ((0, np.nan), (3, np.inf), (7, -np.inf), (8 + 7, np.nan)):
        r = bones.copy()
        r.reshape(-1)[k] = value
        rc, msg = code(ds.handle, skin.handle, r)
        assert rc == bad and f"bone {k // 8} has a non-finite member" in msg, msg
    # a skin for another scene's counts
    import scene_update_cases as cases

    fewer = cases.copy(flat0, **{k: getattr(flat0, k)[:-1] for k in S.TRI_OUT + ("tri_material",)})
    other = DeviceScene(fewer, 0)
    rc, msg = code(other.handle, skin.handle, bones)
    assert rc == bad and "the skin is for n_triangles 41" in msg and "the scene has 40" in msg
    rc = lib.rt_skin_apply_device(other.handle, skin.handle, C.c_void_p(256), None, None)  # (refused before the pointer is used)
    assert rc == bad and "the skin is for n_triangles" in lib.rt_last_error().decode()
    # what rt_scene_update_device refuses: a split-clipped tree, a progressive render
    big = cases.flat_test_scene()
    clipped = DeviceScene(big, 0, bvh=dict(split_depth=8, split_gain=0.99))
    assert clipped.bvh_info()["n_references"] > big.n_triangles, "the builder changed: choose another scene to clip"
    m = S.seeded_mesh(30, 5, 2, True)
    m.update(tri_first=3, n_triangles=big.n_triangles)
    on_clipped = new_skin(clipped, m)
    rc, msg = code(clipped.handle, on_clipped.handle, S.identity_bones(2))
    assert rc == _abi.RT_ERR_UNSUPPORTED and "split clipping" in msg
    S.assert_same_words(on_clipped.geometry(), S.restated(m), what="the kernels did not run")
    p, keep = _abi.make_params(cfg)
    buf = np.zeros(cfg.width * cfg.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 64, C.byref(h)))
    rc, msg = code(ds.handle, skin.handle, bones)
    _lib.check(lib.rt_render_end(h, None))
    assert rc == bad and "progressive" in msg
    assert assert_same_frame(before, render(cfg, ds), "a refused apply changes nothing")
    S.assert_same_words(skin.geometry(), rest, what="... not the skin's arrays either")
    S.assert_same_words(rest, S.restated(mesh), what="the rest mesh")
    with pytest.raises(ValueError):
        skin.apply(bones[:1])
    skin.close(), on_clipped.close(), ds.close(), other.close(), clipped.close()


# ---- 12. the C example ------------------------------------------------------------------------------------------------------------------------
def test_c_skin_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_skin_example"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_skin_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame 4 restores the checksum of the rest frame" in out.stdout and "sah" in out.stdout and "rebuilt" in out.stdout
