"""Ambient-occlusion queries on the GPU: every plane of DeviceScene.ambient_occlusion equals rt_ambient_occlusion_model -- the
linear scan on the host -- bit for bit, on every scene, at every sample count around the segment and round boundaries, with both
flag values, every kind of max_distance, both biases, with and without start rows; at batch sizes around the wavefront and the
workgroup; with every single output plane missing; the result does not depend on the tree (update, rebuild, PLOC rebuild, split
clipping); torch device tensors on a stream of their own give the numpy path's bits; a chain on the device, cast_rays ->
ambient_occlusion, equals the host-staged chain; a call beside a render of the same scene leaves the frame's bits unchanged; the C
example runs."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DeviceScene, Occlusion

import occlusion_cases as oc
import scene_update_cases as upd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _scene(name):
    if name not in _cache:
        flat = oc.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def _planes(got):
    """Occlusion (numpy or tensors) -> the dict of planes of occlusion_cases"""
    out = {}
    for name in oc.PLANES:
        a = getattr(got, name)
        if a is not None and not isinstance(a, np.ndarray):
            a = a.cpu().numpy()
        out[name] = None if a is None else a.view(np.uint32 if name in ("bits", "clear") else a.dtype)
    return out


def _assert_equal(got, want, what):
    got = _planes(got) if isinstance(got, Occlusion) else got
    for name in oc.PLANES:
        g, w = got[name], want[name]
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.size == 0:
            continue
        gb, wb = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        bad = np.flatnonzero((gb != wb).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} points, first {bad[:5]}: got {g[bad[:2]]} want {w[bad[:2]]}"


def _device(ds, p, nrm, s, tab, first=None, bias=1e-4, max_d=np.inf, pt=False, bits=True):
    return ds.ambient_occlusion(p, nrm, samples=s, table=tab, first=first, bias=bias, max_distance=max_d, pass_transmissive=pt, bits=bits)


@pytest.mark.parametrize("s", oc.S_LIST)
@pytest.mark.parametrize("name", oc.SCENES)
def test_every_plane_equals_the_model_bit_for_bit(name, s):
    """n = 493 points: a partial tail wavefront at every S <= 64.  Every combination of the two flag values and the five kinds of
    max_distance, the bias and the start rows alternating along them.  On text_lowres (1687 triangles, where the model's linear
    scan of 493 x S rays takes seconds) the two walking kinds pair with one flag value each, and above S = 64 -- one point per
    wavefront, so the size of the batch maps to nothing in the kernel -- every fourth point is taken."""
    flat, ds = _scene(name)
    p, nrm = oc.points(name)
    tab, first = oc.table(), oc.first(p.shape[0])
    heavy = name == "text_lowres"
    if heavy and s > 64:
        live = p.shape[0] - oc.N_DEAD
        keep = np.r_[np.arange(0, live, 4), np.arange(live, p.shape[0])]  # (the dead points at the end stay)
        p, nrm, first = (np.ascontiguousarray(a[keep]) for a in (p, nrm, first))
    for k, (pt, kind) in enumerate(itertools.product((False, True), oc.MAX_D)):
        if heavy and (pt, kind) in ((True, "inf"), (False, "fraction")):
            continue
        bias, f = oc.BIASES[k % 2], first if k % 3 else None
        max_d = oc.max_distance(kind, flat)
        want = oc.model(flat, p, nrm, s, tab, f, bias, max_d, pt)
        _assert_equal(_device(ds, p, nrm, s, tab, f, bias, max_d, pt), want, f"{name} S {s} pass {pt} max_distance {kind} bias {bias}")


@pytest.mark.parametrize("s", (1, 33, 256))
@pytest.mark.parametrize("n", (0, 1, 63, 65, 257))
def test_small_batches_and_missing_planes(n, s):
    flat, ds = _scene("test_scene")
    p, nrm = oc.points("test_scene")
    p, nrm = p[100:100 + n].copy(), nrm[100:100 + n].copy()
    tab, first = oc.table(), oc.first(n)
    got = _device(ds, p, nrm, s, tab, first)
    assert got.clear.shape == (n,) and got.bits.shape == (n, (s + 31) // 32) and got.bent_normal.shape == (n, 3)
    want = oc.model(flat, p, nrm, s, tab, first, 1e-4)
    _assert_equal(got, want, f"n = {n}, S = {s}")
    if n == 0:
        return
    # one plane missing at a time: it is not written, the three others are, each between guard words
    lib = _lib.load()
    for missing in oc.PLANES:
        guarded = {m: np.full(a.size + 8, 0x5A5A5A5A, np.uint32) for m, a in want.items()}
        views = {m: guarded[m][4:-4].view(want[m].dtype).reshape(want[m].shape) for m in want}
        b = oc.batch_struct(p, nrm, s, tab, first, 1e-4)
        o = oc.out_struct(views, only=[m for m in oc.PLANES if m != missing])
        _lib.check(lib.rt_ambient_occlusion(ds.handle, C.byref(b), C.byref(o)))
        for m in want:
            assert (guarded[m][:4] == 0x5A5A5A5A).all() and (guarded[m][-4:] == 0x5A5A5A5A).all(), (missing, m)
            if m == missing:
                assert (guarded[m] == 0x5A5A5A5A).all(), missing
            else:
                assert np.array_equal(views[m].view(np.uint32), want[m].view(np.uint32)), (missing, m)


def test_result_does_not_depend_on_the_tree():
    name = "text_lowres"
    flat = oc.scene(name)
    p, nrm = oc.points(name)
    tab, first = oc.table(), oc.first(p.shape[0])
    ds = DeviceScene(flat, 0)
    split = DeviceScene(flat, 0, bvh={"split_depth": 3})
    try:
        assert split.bvh_info()["n_references"] > flat.n_triangles == ds.bvh_info()["n_references"]
        for s, max_d in ((33, np.inf), (65, oc.max_distance("fraction", flat))):
            plain = _planes(_device(ds, p, nrm, s, tab, first, max_d=max_d))
            _assert_equal(_device(split, p, nrm, s, tab, first, max_d=max_d), plain, f"split clipping, S {s}")
        _assert_equal(_device(split, p, nrm, 33, tab, first, pt=True), oc.model(flat, p, nrm, 33, tab, first, 1e-4, np.inf, True), "split clipping against the model")
        moved = upd.jitter(flat, 0.05)
        ds.update(moved)
        want = oc.model(moved, p, nrm, 33, tab, first, 1e-4)
        refitted = _planes(_device(ds, p, nrm, 33, tab, first))
        _assert_equal(refitted, want, "after update(jittered)")
        wide = _planes(_device(ds, p, nrm, 65, tab, first))
        ds.rebuild()
        _assert_equal(_device(ds, p, nrm, 33, tab, first), refitted, "after rebuild()")
        _assert_equal(_device(ds, p, nrm, 65, tab, first), wide, "after rebuild(), S 65")
        ds.rebuild(method="ploc")
        _assert_equal(_device(ds, p, nrm, 33, tab, first), refitted, "after rebuild(method='ploc')")
        _assert_equal(_device(ds, p, nrm, 65, tab, first), wide, "after rebuild(method='ploc'), S 65")
    finally:
        ds.close()
        split.close()


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no GPU):
# the tests that hand tensors to the library run in a child process of their own, as tests/test_ray_query_gpu.py's do
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_occlusion_gpu as T
T.{name}()
print("CHILD-OK")
"""


def _run_child(name):
    import sys

    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_torch_tensors_and_the_device_chain_give_the_host_path_bits():
    _run_child("torch_tensors_and_the_device_chain")


def test_a_call_beside_a_render_of_the_same_scene():
    _run_child("call_beside_a_render")


def torch_tensors_and_the_device_chain():
    """(in the child process)"""
    import torch

    import multi_hit_cases as mh

    name = "text_lowres"
    flat, ds = _scene(name)
    p, nrm = oc.points(name)
    tab, first = oc.table(), oc.first(p.shape[0])
    max_d = oc.max_distance("fraction", flat)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    want = {s: _planes(_device(ds, p, nrm, s, tab, first, 0.0, max_d, True)) for s in (7, 129)}
    defaults = _planes(ds.ambient_occlusion(p, nrm))
    tp, tn, tt, tf = (torch.from_numpy(a).to(dev) for a in (p, nrm, tab, first.view(np.int32)))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        got = {s: ds.ambient_occlusion(tp, tn, samples=s, table=tt, first=tf, bias=0.0, max_distance=max_d, pass_transmissive=True, bits=True) for s in (7, 129)}
        plain = ds.ambient_occlusion(tp, tn)  # the default table, uploaded on this stream; no bit plane
    stream.synchronize()
    for s in (7, 129):
        assert got[s].clear.device == tp.device and got[s].clear.dtype == torch.int32 and got[s].bits.dtype == torch.int32
        _assert_equal(got[s], want[s], f"tensors, S {s}")
    assert plain.bits is None and defaults["bits"] is None
    _assert_equal(plain, defaults, "tensors, defaults")
    with pytest.raises(ValueError):
        ds.ambient_occlusion(tp, tn, samples=257)
    with pytest.raises(ValueError):
        ds.ambient_occlusion(tp, tn, first=tf.cpu())
    # the chain on the device: the hit planes of cast_rays go into ambient_occlusion as they are
    o, d = mh.rays(name)
    hits = ds.cast_rays(o, d)
    staged = _planes(ds.ambient_occlusion(hits.point, hits.normal, samples=33, bits=True))
    assert (hits.id < 0).any() and (staged["clear"][hits.id < 0] == 0).all()  # (a miss has the normal 0: a dead point)
    with torch.cuda.stream(stream):
        th = ds.cast_rays(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev))
        chained = ds.ambient_occlusion(th.point, th.normal, samples=33, bits=True)
    stream.synchronize()
    _assert_equal(chained, staged, "device chain")
    ds.close()


def call_beside_a_render():
    """(in the child process) as tests/test_ray_query_gpu.py's query beside a render"""
    import torch

    import ray_query_cases as rq
    from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig
    from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import RaytracerRenderer

    cfg = RenderConfig.from_features(["anti_aliasing", "soft_shadows", "reflections", "refractions"])
    _, flat = rq.scene("test_scene")
    r = RaytracerRenderer(cfg, device=0)
    ds = r.device_scene(flat)
    rng = np.random.default_rng(4)
    p0, n0 = oc.points("test_scene")
    pick = rng.integers(0, p0.shape[0], 60000)
    p, nrm = np.ascontiguousarray(p0[pick]), np.ascontiguousarray(n0[pick])
    solo = _planes(ds.ambient_occlusion(p, nrm, samples=64, bits=True))
    lib = _lib.load()
    prm, keep = _abi.make_params(cfg)
    dev = torch.device("cuda", 0)
    npx = cfg.width * cfg.height
    s_render, s_query = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    argb_solo = torch.zeros(npx, dtype=torch.int32, device=dev)
    _lib.check(lib.rt_render_device(ds.handle, C.byref(prm), argb_solo.data_ptr(), None, C.c_void_p(s_render.cuda_stream)))
    s_render.synchronize()
    argb = torch.zeros(npx, dtype=torch.int32, device=dev)
    tp, tn = torch.from_numpy(p).to(dev), torch.from_numpy(nrm).to(dev)
    tab = torch.from_numpy(_default_table(64)).to(dev)
    torch.cuda.synchronize()
    _lib.check(lib.rt_render_device(ds.handle, C.byref(prm), argb.data_ptr(), None, C.c_void_p(s_render.cuda_stream)))
    with torch.cuda.stream(s_query):
        got = ds.ambient_occlusion(tp, tn, samples=64, table=tab, bits=True)
    torch.cuda.synchronize()
    assert torch.equal(argb, argb_solo)
    _assert_equal(got, solo, "beside a render")


def _default_table(s):
    from hslu_i.ba_raytracing.f2501_raytracer_amd import sampling

    return sampling.hemisphere_samples(s)


def test_c_ambient_occlusion_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_ambient_occlusion_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_ambient_occlusion_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device equals model: yes" in out.stdout and "model checksum" in out.stdout and "device checksum" in out.stdout
