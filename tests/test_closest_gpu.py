"""Closest-point queries on the GPU: every plane of DeviceScene.closest_points equals rt_closest_points_model -- the linear
scan on the host -- bit for bit, on every scene, with and without radii, at batch sizes around the wavefront and the
workgroup; NULL planes are not written; the result does not depend on the tree (update, rebuild, PLOC rebuild); torch device
tensors on a stream of their own give the numpy path's bits; the C example runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import ClosestPoints, DeviceScene

import closest_cases as cc
import scene_update_cases as upd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _scene(name):
    if name not in _cache:
        flat = cc.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _planes(got):
    return {name: np.asarray(getattr(got, name)).astype(dt, copy=False) for name, dt, _ in cc.PLANES}


def _assert_equal(got, want, what):
    got = _planes(got) if isinstance(got, ClosestPoints) else got
    for name, _, _ in cc.PLANES:
        g, w = np.ascontiguousarray(got[name]).view(np.uint32), np.ascontiguousarray(want[name]).view(np.uint32)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.size == 0:
            continue
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} points, first {bad[:5]}: got {got[name][bad[:3]]} want {want[name][bad[:3]]}"


@pytest.mark.parametrize("name", cc.SCENES)
def test_every_plane_equals_the_model_bit_for_bit(name):
    flat, ds = _scene(name)
    n = 5000 if name == "text" else 20000  # (20000: not a multiple of 256)
    pts = cc.points(flat, n, seed=41)
    for r in (None, cc.mixed_radii(flat, pts, seed=42)):
        want = cc.model(flat, pts, r)
        _assert_equal(ds.closest_points(pts, r), want, f"{name}, radii {r is not None}")
        if name in ("test_scene", "text_lowres"):
            assert (want["id"] >= 0).sum() > n // 4 and len(np.unique(want["id"])) > 3


@pytest.mark.parametrize("n", (0, 1, 63, 65, 257))
def test_small_batches(n):
    flat, ds = _scene("test_scene")
    pts = cc.points(flat, 300, seed=43)[:n]
    got = ds.closest_points(pts)
    assert got.id.shape == (n,) and got.point.shape == (n, 3) and got.bary.shape == (n, 2)
    _assert_equal(got, cc.model(flat, pts), f"n = {n}")


def test_a_null_plane_is_not_written():
    flat, ds = _scene("test_scene")
    n = 1000
    pts = cc.points(flat, n, seed=44)
    want = cc.model(flat, pts)
    lib = _lib.load()
    for keep in ("id", "distance", "point", "normal", "bary", "material"):
        # one plane at a time, in the middle of an array of guard bytes
        out = cc.new_planes(n)
        guard = {name: np.full(out[name].size + 64, 0xA5A5A5A5, np.uint32) for name in out}
        h = _abi.rt_point_hits()
        setattr(h, keep, guard[keep].ctypes.data + 128)
        b = cc.batch_struct(pts, None)
        _lib.check(lib.rt_closest_points(ds.handle, C.byref(b), C.byref(h)))
        body = guard[keep][32:32 + out[keep].size]
        assert np.array_equal(body, np.ascontiguousarray(want[keep]).view(np.uint32).ravel()), keep
        assert (guard[keep][:32] == 0xA5A5A5A5).all() and (guard[keep][32 + out[keep].size:] == 0xA5A5A5A5).all(), keep


def test_result_does_not_depend_on_the_tree():
    flat = cc.scene("text_lowres")
    ds = DeviceScene(flat, 0)
    try:
        pts = cc.points(flat, 20000, seed=45)
        r = cc.mixed_radii(flat, pts, seed=46)
        moved = upd.jitter(flat, 0.05)
        ds.update(moved)
        want = cc.model(moved, pts, r)
        refitted = ds.closest_points(pts, r)
        _assert_equal(refitted, want, "after update(jittered)")
        ds.rebuild()
        _assert_equal(ds.closest_points(pts, r), _planes(refitted), "after rebuild()")
        ds.rebuild(method="ploc")
        _assert_equal(ds.closest_points(pts, r), _planes(refitted), "after rebuild(method='ploc')")
    finally:
        ds.close()


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no GPU):
# the test that hands tensors to the library runs in a child process of its own, as tests/test_ray_query_gpu.py's do
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_closest_gpu as T
T.torch_tensors_on_their_own_stream()
print("CHILD-OK")
"""


def test_torch_tensors_on_their_own_stream_give_the_same_bits():
    import sys

    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def torch_tensors_on_their_own_stream():
    """(in the child process)"""
    import torch

    flat, ds = _scene("text_lowres")
    pts = cc.points(flat, 20000, seed=47)
    r = cc.mixed_radii(flat, pts, seed=48)
    want = _planes(ds.closest_points(pts, r))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    tp, tr = torch.from_numpy(pts).to(dev), torch.from_numpy(r).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        got = ds.closest_points(tp, tr)
        free = ds.closest_points(tp)
    stream.synchronize()
    assert got.id.device == tp.device and got.material.dtype == torch.int32
    as_np = {name: getattr(got, name).cpu().numpy().view(dt) for name, dt, _ in cc.PLANES}
    _assert_equal(as_np, want, "tensors")
    _assert_equal({name: getattr(free, name).cpu().numpy().view(dt) for name, dt, _ in cc.PLANES}, cc.model(flat, pts), "tensors, no radii")
    ds.close()


def test_c_closest_points_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_closest_points_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_closest_points_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device equals model: yes, checksum" in out.stdout
