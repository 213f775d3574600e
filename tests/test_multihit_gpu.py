"""Multi-hit ray queries on the GPU: every plane of DeviceScene.list_intersections, count and total included, equals
rt_list_intersections_model -- the linear scan on the host -- bit for bit, on every scene, with and without culling, for every
K class and kind of max_distance, at batch sizes around the wavefront and the workgroup; entry 0 is cast_rays' answer;
count_intersections is the model's total; the result does not depend on the tree (update, rebuild, PLOC rebuild, split
clipping); chained calls page through every hit; torch device tensors on a stream of their own give the numpy path's bits; the
C example runs."""
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, RayHitLists

import multi_hit_cases as mh
import scene_update_cases as upd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("test_scene", "spheres", "triangles", "empty", "text_lowres")
NAMES = ("count", "total") + tuple(name for name, _, _ in mh.LIST_PLANES)
_cache = {}


def _scene(name):
    if name not in _cache:
        flat = mh.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _planes(got):
    """RayHitLists (numpy or tensors) -> the dict of planes of multi_hit_cases"""
    out = {}
    for name in NAMES:
        a = getattr(got, name)
        if a is not None and not isinstance(a, np.ndarray):
            a = a.cpu().numpy()
        out[name] = None if a is None else a.view(np.uint32 if name in ("count", "total", "material") else a.dtype)
    return out


def _assert_equal(got, want, what):
    got = _planes(got) if isinstance(got, RayHitLists) else got
    for name in NAMES:
        g, w = got[name], want[name]
        assert (g is None) == (w is None), (what, name)
        if g is None or g.size == 0:
            assert g is None or g.shape == w.shape, (what, name)
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        gb, wb = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        bad = np.flatnonzero((gb != wb).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} rays, first {bad[:5]}: got {g[bad[:2]]} want {w[bad[:2]]}"


def _device(ds, o, d, k, max_d=None, cull=False, after=None, total=True):
    return ds.list_intersections(o, d, max_hits=k, max_distance=max_d, backface_culling=cull, total=total, after=after)


@pytest.mark.parametrize("cull", (False, True))
@pytest.mark.parametrize("name", SCENES)
def test_every_plane_equals_the_model_bit_for_bit(name, cull):
    flat, ds = _scene(name)
    o, d = mh.rays(name)  # n = 1021: a partial tail wavefront
    for k in mh.KS:
        want = mh.model(flat, o, d, k, cull=cull)
        _assert_equal(_device(ds, o, d, k, cull=cull), want, f"{name} cull {cull} K {k}")
        if k == 1:  # entry 0 is cast_rays' answer
            near = ds.cast_rays(o, d, backface_culling=cull)
            for plane in ("id", "t", "point", "normal", "material"):
                assert np.array_equal(np.ascontiguousarray(getattr(near, plane)).view(np.uint32).ravel(), want[plane].view(np.uint32).ravel()), plane
        if k == 16:
            assert np.array_equal(ds.count_intersections(o, d, backface_culling=cull), want["total"])
    second = mh.model(flat, o, d, 2, cull=cull)["t"][:, 1].copy()
    for kind in mh.MAX_D[1:]:
        m = mh.max_distance(kind, flat, o, second)
        _assert_equal(_device(ds, o, d, 5, m, cull), mh.model(flat, o, d, 5, m, cull), f"{name} cull {cull} max_distance {kind}")
        _assert_equal(_device(ds, o, d, 2, m, cull, total=False), mh.model(flat, o, d, 2, m, cull, total=False), f"{name} cull {cull} {kind}, no total")
    m = mh.max_distance("mixed", flat, o, second)
    assert np.array_equal(ds.count_intersections(o, d, m, cull), mh.model(flat, o, d, 16, m, cull)["total"])
    if name in ("test_scene", "text_lowres") and not cull:  # the ray set is not degenerate
        total = mh.model(flat, o, d, 16)["total"]
        assert (total >= 2).mean() >= 0.40 and (total > 4).mean() >= 0.05


@pytest.mark.parametrize("n", (0, 1, 63, 65, 257))
def test_small_batches(n):
    flat, ds = _scene("test_scene")
    o, d = mh.rays("test_scene")
    o, d = o[100:100 + n].copy(), d[100:100 + n].copy()
    for k in (4, 5):  # (one K of each list class)
        got = _device(ds, o, d, k)
        assert got.count.shape == (n,) and got.id.shape == (n, k) and got.point.shape == (n, k, 3)
        _assert_equal(got, mh.model(flat, o, d, k), f"n = {n}, K = {k}")


def test_result_does_not_depend_on_the_tree():
    flat = mh.scene("text_lowres")
    o, d = mh.rays("text_lowres")
    ds = DeviceScene(flat, 0)
    split = DeviceScene(flat, 0, bvh={"split_depth": 3})
    try:
        # (n_references is a field of rt_bvh_info, which rt_scene_bvh_info fills)
        assert split.bvh_info()["n_references"] > flat.n_triangles == ds.bvh_info()["n_references"]
        for k in (4, 16):
            _assert_equal(_device(split, o, d, k), _planes(_device(ds, o, d, k)), f"split clipping, K {k}")
            _assert_equal(_device(split, o, d, k, cull=True), mh.model(flat, o, d, k, cull=True), f"split clipping, culling, K {k}")
        moved = upd.jitter(flat, 0.05)
        ds.update(moved)
        want = mh.model(moved, o, d, 16)
        refitted = _planes(_device(ds, o, d, 16))
        _assert_equal(refitted, want, "after update(jittered)")
        ds.rebuild()
        _assert_equal(_device(ds, o, d, 16), refitted, "after rebuild()")
        ds.rebuild(method="ploc")
        _assert_equal(_device(ds, o, d, 16), refitted, "after rebuild(method='ploc')")
    finally:
        ds.close()
        split.close()


def test_paging_on_the_device():
    # the hand-made scene at K = 16: 42 layers under one ray, the coincident pair in order
    flat, ds = _scene("layers")
    ids, ts = mh.layers_answer()
    o, d = np.tile(np.float32(mh.LAYER_ORIGIN), (3, 1)), np.tile(np.float32(mh.LAYER_DIR), (3, 1))
    keys, first = mh.chain(lambda after: _planes(_device(ds, o, d, 16, after=after)), 3, 16)
    assert first["total"].tolist() == [42, 42, 42]
    for row in keys:
        assert [key[1] for key in row] == ids and np.array([key[0] for key in row], np.uint32).view(np.float32).tolist() == ts
    # test_scene at K = 2: the chained calls give the model's full lists
    flat, ds = _scene("test_scene")
    o, d = mh.rays("test_scene")
    full = mh.model(flat, o, d, 16)
    assert int(full["total"].max()) <= 16
    keys, first = mh.chain(lambda after: _planes(_device(ds, o, d, 2, after=after)), o.shape[0], 2)
    assert np.array_equal(first["total"], full["total"])
    for i in range(o.shape[0]):
        c = int(full["total"][i])
        assert keys[i] == list(zip(full["t"][i, :c].view(np.uint32).tolist(), full["id"][i, :c].tolist())), i


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no GPU):
# the test that hands tensors to the library runs in a child process of its own, as tests/test_ray_query_gpu.py's do
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_multihit_gpu as T
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
    o, d = mh.rays("text_lowres")
    m = mh.max_distance("mixed", flat, o)
    first = _planes(_device(ds, o, d, 4))
    has = first["count"] > 0
    rows, last = np.arange(o.shape[0]), np.maximum(first["count"].astype(np.int64) - 1, 0)
    after = (np.where(has, first["t"][rows, last], np.float32(np.inf)).astype(np.float32), np.where(has, first["id"][rows, last], -1).astype(np.int32))
    want = _planes(_device(ds, o, d, 4, m, True, after))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    to, td, tm, tat, tai = (torch.from_numpy(a).to(dev) for a in (o, d, m, after[0], after[1]))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        got = ds.list_intersections(to, td, max_hits=4, max_distance=tm, backface_culling=True, total=True, after=(tat, tai))
        free = ds.list_intersections(to, td, max_hits=16)
        counted = ds.count_intersections(to, td)
    stream.synchronize()
    assert got.id.device == to.device and got.material.dtype == torch.int32 and got.count.dtype == torch.int32 and free.total is None
    _assert_equal(got, want, "tensors")
    model = mh.model(flat, o, d, 16)
    _assert_equal(free, dict(model, total=None), "tensors, K = 16, no total")
    assert np.array_equal(counted.cpu().numpy().view(np.uint32), model["total"])
    ds.close()


def test_c_list_intersections_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_list_intersections_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_list_intersections_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device equals model: yes" in out.stdout and "layers under the ray: 42" in out.stdout
