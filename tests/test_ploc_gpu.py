"""PLOC rebuilds and RT_REBUILD_KEEP_BETTER on the GPU, through Python and the C ABI (rt_scene_rebuild_with, csrc/rt_rebuild.cpp):
a handle whose tree has been rebuilt with PLOC renders and answers queries as a handle freshly created from the same
geometry -- hit ids and distances the same bits, colours within the project's bar RGB_TOL (the shadow products of a pixel
may be summed in another leaf-slot order) -- and what it reports about its tree, the SAH sums of the report included, is the
host model's (tests/test_ploc_host.py), the integers bit for bit."""
import ctypes as C

import numpy as np
import pytest

import f64_query_cases as fq
import ploc_cases as pc
import scene_update_cases as cases
import skin_cases as S
from test_ploc_host import probe, rebuilt_ploc  # noqa: F401  (probe: the host-only fixture)
from test_pose_gpu import new_pose, posed_flat, posed_scene
from test_rebuild_gpu import EVERYTHING, RAYS, assert_equivalent_frame, bits, deformed
from test_rebuild_host import info_of, sah_of
from test_scene_update_gpu import CONFIGS, RGB_TOL, SCENES, WINDOWS, assert_same_frame, render
from test_scene_update_host import pack, refit
from test_skin_gpu import new_skin
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene

pytestmark = pytest.mark.gpu
TREE = ("n_nodes", "n_leaves", "max_depth", "max_leaf_size", "n_references", "bytes_nodes", "bytes_triangles")


def assert_equivalent_rays(ds, fresh, name, what):
    """cast_rays ids and t on the 1021 seeded rays are the bits of the fresh handle's, any_intersection likewise"""
    o, d, kind, max_d = fq.rays(RAYS[name])
    assert len(o) == 1021
    hits, want = ds.cast_rays(o, d), fresh.cast_rays(o, d)
    for a, b, field in zip(hits, want, hits._fields):
        assert np.array_equal(bits(a), bits(b)), f"{what}: cast_rays.{field}"
    assert (hits.id >= 0).sum() > 200, "the rays meet the scene"
    occ, want = ds.any_intersection(o, d, max_d), fresh.any_intersection(o, d, max_d)
    assert np.array_equal(occ.has_intersection, want.has_intersection) and np.array_equal(occ.completely_occluded, want.completely_occluded), what
    assert np.abs(occ.combined_opacity - want.combined_opacity).max() <= RGB_TOL, f"{what}: any_intersection.combined_opacity"


def assert_equivalent_frames(ds, fresh, name, what):
    for c in ("direct", "soft"):
        assert_equivalent_frame(render(CONFIGS[c](), ds, WINDOWS[name]), render(CONFIGS[c](), fresh, WINDOWS[name]), f"{what} / {c}")


# ---- 1. a PLOC handle against a fresh one, and against the host model ------------------------------------------------------------
@pytest.mark.parametrize("case", ["fresh", "deformed"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ploc_handle_answers_as_a_fresh_one(probe, name, case):  # noqa: F811
    flat = SCENES[name]()
    now = deformed(name, flat) if case == "deformed" else flat
    what = f"{name} / {case}"
    ds = DeviceScene(flat, 0)
    created = ds.bvh_quality()
    if now is not flat:
        ds.update(now)
    refitted = ds.bvh_quality()
    rep = ds.rebuild(info=True, method="ploc")
    fresh = DeviceScene(now, 0)
    # the host model of the same history
    pack(probe, 0, flat)
    if now is not flat:
        assert refit(probe, 0, flat, now) == 0, probe.probe_error()
    _, _, iterations = rebuilt_ploc(probe, now)
    want = info_of(probe, 0)
    sums, sah, bad = sah_of(probe, 0)
    assert rep["swapped"] == 1 and rep["tables_invalidated"] == EVERYTHING and rep["device_ms"] > 0 and rep["iterations"] == iterations
    assert {k: rep[k] for k in TREE[:4]} == {k: want[k] for k in TREE[:4]}
    assert (rep["inner_q_after"], rep["leaf_q_after"]) == sums and rep["sah_after"] == sah, "the candidate's integer SAH sums, bit for bit"
    assert (rep["inner_q_before"], rep["leaf_q_before"]) == (refitted["inner_q"], refitted["leaf_q"]) and rep["sah_before"] == refitted["sah_now"]
    bi = ds.bvh_info()
    assert {k: bi[k] for k in TREE} == {k: want[k] for k in TREE}
    assert ds.memory_info()["bytes_bvh"] == want["bytes_bvh"]
    q = ds.bvh_quality()
    assert (q["inner_q"], q["leaf_q"], q["n_bad"]) == (sums[0], sums[1], bad)
    assert q["sah_now"] == sah and q["sah_created"] == created["sah_created"], "sah_created stays the value of creation"
    print(f"{what}: PLOC rebuild {rep['total_ms']:.3f} ms wall, {rep['device_ms']:.3f} ms device, {rep['iterations']} iterations; {rep['n_nodes']} nodes, "
          f"depth {rep['max_depth']}; SAH created {created['sah_created']:.2f}, refitted {refitted['sah_now']:.2f}, PLOC {q['sah_now']:.2f}")
    assert_equivalent_rays(ds, fresh, name, what)
    assert_equivalent_frames(ds, fresh, name, what)
    ds.close(), fresh.close()


# ---- 2. updates, poses, skins and a second rebuild on a PLOC tree ------------------------------------------------------------------
def test_update_pose_and_second_rebuild_after_ploc_match_fresh_handles():
    name = "semesterbild"
    flat0, rest, parts, steps = posed_scene(name)
    ds = DeviceScene(flat0, 0)
    pose = new_pose(ds, rest, parts)
    ds.rebuild(method="ploc")
    moved = cases.jitter(flat0, 0.05)
    info = ds.update(moved, info=True)
    assert info["nodes_refitted"] == ds.bvh_info()["n_nodes"] and info["slots_rewritten"] == flat0.n_triangles
    fresh = DeviceScene(moved, 0)
    assert_equivalent_frames(ds, fresh, name, "update after PLOC")
    assert_equivalent_rays(ds, fresh, name, "update after PLOC")
    fresh.close()
    ds.update(flat0)
    rows = steps[1][1]
    pose.apply(rows)
    fresh = DeviceScene(posed_flat(flat0, rest, parts, rows), 0)
    assert_equivalent_frames(ds, fresh, name, "pose after PLOC")
    rep = ds.rebuild(info=True, method="ploc", radius=16)
    assert rep["swapped"] == 1 and rep["iterations"] > 0
    assert_equivalent_frames(ds, fresh, name, "a second PLOC rebuild, of the posed scene")
    assert_equivalent_rays(ds, fresh, name, "a second PLOC rebuild, of the posed scene")
    pose.close(), ds.close(), fresh.close()


def test_skin_after_ploc_matches_a_fresh_handle():
    flat0, mesh = S.semesterbild_skin()
    ds = DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    ds.rebuild(method="ploc")
    bones = S.bend(mesh, 20.0)
    skin.apply(bones)  # (the skin speaks in canonical indices: it goes on working on the rebuilt tree)
    fresh = DeviceScene(S.with_mesh(flat0, mesh, bones), 0)
    assert_equivalent_frames(ds, fresh, "semesterbild", "skin after PLOC")
    skin.close(), ds.close(), fresh.close()


# ---- 3. the LBVH through the new entry point ---------------------------------------------------------------------------------------
def test_rebuild_with_lbvh_leaves_the_tree_of_rt_scene_rebuild():
    name = "semesterbild"
    flat = SCENES[name]()
    now = deformed(name, flat)
    a, b = DeviceScene(flat, 0), DeviceScene(flat, 0)
    a.update(now), b.update(now)
    old = a.rebuild(info=True)
    lib = _lib.load()
    desc, rep = _abi.rt_rebuild_desc(_abi.RT_REBUILD_LBVH, 0, 0, 0), _abi.rt_rebuild_report()
    _lib.check(lib.rt_scene_rebuild_with(b.handle, C.byref(desc), C.byref(rep)))
    new = rep.as_dict()
    assert new["swapped"] == 1 and new["iterations"] == 0
    assert {k: new[k] for k in TREE[:4]} == {k: old[k] for k in TREE[:4]} and a.bvh_info() == b.bvh_info()
    qa, qb = a.bvh_quality(), b.bvh_quality()
    assert (qa["inner_q"], qa["leaf_q"], qa["n_bad"]) == (qb["inner_q"], qb["leaf_q"], qb["n_bad"]) == (new["inner_q_after"], new["leaf_q_after"], 0)
    o, d, kind, max_d = fq.rays(RAYS[name])
    for x, y, field in zip(a.cast_rays(o, d), b.cast_rays(o, d), ("id", "t")):
        assert np.array_equal(bits(x), bits(y)), field
    assert assert_same_frame(render(CONFIGS["direct"](), a, WINDOWS[name]), render(CONFIGS["direct"](), b, WINDOWS[name]), "LBVH either way"), "the float planes too"
    assert b.rebuild(info=True, method="lbvh", keep_better=False)["n_nodes"] == old["n_nodes"], "as today: rt_scene_rebuild"
    a.close(), b.close()


# ---- 4. keep-better ----------------------------------------------------------------------------------------------------------------
def test_keep_better_leaves_a_better_tree_in_place():
    """test_scene as created: wall-sized triangles, the binned-SAH tree of creation costs less than any rebuild"""
    name = "test_scene"
    cfg, win = CONFIGS["soft"](), WINDOWS[name]
    ds = DeviceScene(SCENES[name](), 0)
    before, info_before, q_before, mem_before = render(cfg, ds, win), ds.bvh_info(), ds.bvh_quality(), ds.memory_info()
    rep = ds.rebuild(info=True, method="ploc", keep_better=True)
    assert rep["swapped"] == 0 and rep["tables_invalidated"] == 0 and not rep["sah_after"] < rep["sah_before"]
    assert rep["iterations"] > 0 and (rep["inner_q_before"], rep["leaf_q_before"]) == (q_before["inner_q"], q_before["leaf_q"])
    assert {k: rep[k] for k in TREE[:4]} == {k: info_before[k] for k in TREE[:4]}, "info: the tree in place"
    q = ds.bvh_quality()
    assert ds.bvh_info() == info_before and (q["inner_q"], q["leaf_q"], q["sah_now"]) == (q_before["inner_q"], q_before["leaf_q"], q_before["sah_now"])
    after = ds.memory_info()
    assert after["cell_lists_built"] == mem_before["cell_lists_built"] and after["bytes_flags"] == mem_before["bytes_flags"], "receiver tables kept"
    assert assert_same_frame(before, render(cfg, ds, win), "keep-better refused the candidate"), "the float planes too"
    ds.close()


def test_keep_better_takes_a_better_tree():
    created, current = pc.deformed("shuffle")
    ds = DeviceScene(created, 0)
    ds.update(current)
    rep = ds.rebuild(info=True, method="ploc", keep_better=True)
    assert rep["swapped"] == 1 and rep["sah_after"] < rep["sah_before"] and rep["tables_invalidated"] == EVERYTHING
    assert ds.bvh_quality()["sah_now"] == rep["sah_after"]
    fresh = DeviceScene(current, 0)
    assert_equivalent_rays(ds, fresh, "semesterbild", "shuffle, keep-better")
    ds.close(), fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_a_progressive_render_in_flight_refuses_the_call():
    name = "test_scene"
    cfg, win = CONFIGS["direct"](), WINDOWS[name]
    lib = _lib.load()
    ds = DeviceScene(SCENES[name](), 0)
    before, info_before = render(cfg, ds, win), ds.bvh_info()
    p, keep = _abi.make_params(cfg)
    buf = np.zeros(cfg.width * cfg.height, np.uint32)
    h = C.c_void_p()
    _lib.check(lib.rt_render_begin(ds.handle, C.byref(p), buf.ctypes.data, 64, C.byref(h)))
    desc, rep = _abi.rt_rebuild_desc(_abi.RT_REBUILD_PLOC, 0, 0, 0), _abi.rt_rebuild_report()
    rc = lib.rt_scene_rebuild_with(ds.handle, C.byref(desc), C.byref(rep))
    msg = lib.rt_last_error().decode()
    _lib.check(lib.rt_render_end(h, None))
    assert rc == _abi.RT_ERR_INVALID_ARG and "progressive" in msg
    assert ds.bvh_info() == info_before and assert_same_frame(before, render(cfg, ds, win), "refused: progressive render"), "the float planes too"
    with pytest.raises(ValueError):
        ds.rebuild(method="sah")
    ds.close()


def test_the_iteration_cap_leaves_the_handle_as_it_was():
    """a regular strip of 1000 equal triangles (tests/test_ploc_host.py says why): RT_ERR_UNSUPPORTED after 32 read-back batches"""
    import rebuild_cases as rc

    ds = DeviceScene(rc.strip(1000), 0)
    info_before, q_before = ds.bvh_info(), ds.bvh_quality()
    with pytest.raises(_lib.RtError) as e:
        ds.rebuild(method="ploc")
    assert e.value.code == _abi.RT_ERR_UNSUPPORTED and "256 iterations" in str(e.value)
    q = ds.bvh_quality()
    assert ds.bvh_info() == info_before and (q["inner_q"], q["leaf_q"]) == (q_before["inner_q"], q_before["leaf_q"])
    ds.rebuild()  # (the LBVH takes it)
    ds.close()


# ---- 6. the C example ------------------------------------------------------------------------------------------------------------------
def test_c_rebuild_quality_example_runs(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_rebuild_quality_example"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "c_rebuild_quality_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "swapped 1" in out.stdout and "kept the tree in place" in out.stdout
