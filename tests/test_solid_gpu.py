"""Containment and signed-distance queries on the GPU: every plane of rt_signed_distance / rt_contains_points on a handle equals
rt_solid_packed after rt_closest_packed -- the kernels' walks run on the host over a blob packed from the same description (the
twin of tests/test_solid_host.py, which equals the linear-scan model there) -- bit for bit, on every scene, at batch sizes around
the wavefront, with 1, 3 and 8 directions and both rules; the distance planes are rt_closest_points_device's; the handle answers
for what it holds after update, pose, skin and the two rebuilds; a mesh moved away leaves its points outside; numpy arrays and
torch tensors on a stream of their own give the same bits; missing planes stay untouched; a split-clipped handle is refused; the
C example runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.renderer import DevicePose, DeviceScene

import scene_update_cases as upd
import solid_cases as sc
from test_solid_host import pack, packed, probe  # noqa: F401  (the host-only fixture and its calls)

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 63, 64, 65, None)  # None: the full set of 501
_cache = {}


def _scene(name):
    if name not in _cache:
        flat = sc.scene(name)
        _cache[name] = (flat, DeviceScene(flat, 0))
    return _cache[name]


def device(ds, p, dirs, rule="parity", max_d=None, names=sc.SD_PLANES, fill=0xA5):
    """rt_signed_distance on host arrays -> dict of planes (those of `names`; the others are not asked for)"""
    out = sc.new_planes(p.shape[0], dirs.shape[0], names, fill=fill)
    _lib.check(_lib.load().rt_signed_distance(ds.handle, C.byref(sc.batch_struct(p, dirs, rule, max_d)), C.byref(sc.sd_struct(out))))
    return out


def assert_equal(got, want, what):
    for name in want:
        g, w = got[name], want[name]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.size == 0:
            continue
        gb, wb = np.ascontiguousarray(g).view(np.uint8).reshape(g.shape[0], -1), np.ascontiguousarray(w).view(np.uint8).reshape(g.shape[0], -1)
        bad = np.flatnonzero((gb != wb).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} points, first {bad[:5]}: got {g[bad[:2]]} want {w[bad[:2]]}"


@pytest.mark.parametrize("r", sc.TABLES)
@pytest.mark.parametrize("name", sc.SCENES)
def test_every_plane_equals_the_host_twin_bit_for_bit(probe, name, r):  # noqa: F811
    flat, ds = _scene(name)
    pack(probe, flat)
    full, dirs = sc.points(name), sc.table(r)
    for k, n in enumerate(SIZES):
        # (the short batches end with the dead points too)
        p = full if n is None else np.ascontiguousarray(full[full.shape[0] - n:])
        for rule in sc.RULES:
            max_d = sc.max_distance(flat, p.shape[0]) if (k + (rule == "winding")) % 2 else None
            want = packed(probe, p, dirs, rule, max_d)
            got = device(ds, p, dirs, rule, max_d)
            assert_equal(got, want, f"{name} R {r} n {p.shape[0]} {rule}")
            if p.shape[0]:
                only = sc.new_planes(p.shape[0], r, sc.SOLID_PLANES, fill=0xA5)
                _lib.check(_lib.load().rt_contains_points(ds.handle, C.byref(sc.batch_struct(p, dirs, rule)), C.byref(sc.solid_struct(only))))
                assert_equal(only, {m: want[m] for m in sc.SOLID_PLANES}, f"{name} R {r} n {p.shape[0]} {rule}: rt_contains_points")


def test_missing_planes_stay_untouched():
    flat, ds = _scene("ico")
    p, dirs = np.ascontiguousarray(sc.points("ico")[-65:]), sc.table(3)
    max_d = sc.max_distance(flat, 65)
    want = device(ds, p, dirs, "winding", max_d)
    lib = _lib.load()
    for missing in sc.SD_PLANES:
        guarded = {m: np.full((a.nbytes + 3) // 4 + 8, 0x5A5A5A5A, np.uint32) for m, a in want.items()}
        views = {m: guarded[m][4:-4].view(np.uint8)[:want[m].nbytes].view(want[m].dtype).reshape(want[m].shape) for m in want}
        o = sc.sd_struct(views, only=[m for m in sc.SD_PLANES if m != missing])
        _lib.check(lib.rt_signed_distance(ds.handle, C.byref(sc.batch_struct(p, dirs, "winding", max_d)), C.byref(o)))
        for m in want:
            assert (guarded[m][:4] == 0x5A5A5A5A).all() and (guarded[m][-4:] == 0x5A5A5A5A).all(), (missing, m)
            if m == missing:
                assert (guarded[m] == 0x5A5A5A5A).all(), missing
            else:
                assert np.array_equal(views[m].view(np.uint8), want[m].view(np.uint8)), (missing, m)


# ---- the handle answers for what it holds ----------------------------------------------------------------------------------------
class Twin:
    """the packed blob on the host that follows a handle: packed from its description, refitted to what the handle holds after
    an update, a pose or a skin, rebuilt when it is rebuilt"""

    def __init__(self, lib, flat):
        self.lib, self.flat = lib, flat
        pack(lib, flat)

    def follow(self, new):
        delta, keep = _abi.make_scene_delta(new, _abi.scene_delta_groups(self.flat, new))
        assert self.lib.probe_refit(C.byref(delta)) == 0, self.lib.probe_error()
        self.flat = new

    def rebuild(self, ploc):
        counts = np.zeros(4, np.uint32)
        assert self.lib.probe_rebuild(C.c_uint32(ploc), C.c_void_p(counts.ctypes.data)) == 0, self.lib.probe_error()

    def check(self, ds, p, what):
        for r, rule, with_max_d in ((3, "parity", False), (8, "winding", True)):
            max_d = sc.max_distance(self.flat, p.shape[0]) if with_max_d else None
            assert_equal(device(ds, p, sc.table(r), rule, max_d), packed(self.lib, p, sc.table(r), rule, max_d), f"{what}, R {r} {rule}")


def test_update_pose_and_rebuilds_on_one_handle(probe):  # noqa: F811
    from hslu_i.ba_raytracing.f2501_raytracer_amd.f32math import Rotor3, Similarity3, Vec3

    flat = sc.ico_flat()
    p = sc.points("ico")
    ds = DeviceScene(flat, 0)
    twin = Twin(probe, flat)
    try:
        twin.check(ds, p, "as created")
        before = device(ds, p, sc.table(3))
        moved = upd.jitter(flat, 0.05)
        ds.update(moved)
        twin.follow(moved)
        twin.check(ds, p, "after update(jittered)")
        assert sc.same_bits(device(ds, p, sc.table(3)), before) != []  # (the jitter shows)
        ds.rebuild()
        twin.rebuild(0)
        twin.check(ds, p, "after rebuild()")
        # the icosphere and the sphere beside it as one rigid part, turned and moved
        pose = DevicePose(ds, [(0, flat.n_triangles, 0, 1)])
        t = Similarity3.new(Vec3.new(F32(0.25), F32(-0.125), F32(0.5)), Rotor3.from_rotation_xy(F32(0.3)), F32(1.25))
        pose.apply([t])
        twin.follow(ds.flat)
        twin.check(ds, p, "after DevicePose.apply")
        ds.rebuild(method="ploc")
        twin.rebuild(1)
        twin.check(ds, p, "after rebuild(method='ploc')")
        pose.close()
    finally:
        ds.close()


def test_skin_apply_on_a_small_mesh(probe):  # noqa: F811
    import skin_cases as S
    from test_skin_gpu import new_skin

    flat0, mesh = S.strip_scene()
    ds = DeviceScene(flat0, 0)
    skin = new_skin(ds, mesh)
    twin = Twin(probe, flat0)
    p = np.ascontiguousarray(np.concatenate([sc.free_points(flat0, 7, 253), sc.points("empty")[sc.DEAD]]), F32)
    try:
        for label, bones in S.four_steps(mesh)[:2]:
            skin.apply(bones)
            twin.follow(ds.flat)
            twin.check(ds, p, f"after DeviceSkin.apply ({label})")
        skin.close()
    finally:
        ds.close()


def test_a_mesh_moved_away_leaves_its_points_outside():
    from test_solid_host import ico_points

    p, dist = ico_points()
    was_in = dist <= 0.9 * sc.ico_inradius() + 1e-6
    ds = DeviceScene(sc.ico_flat(), 0)
    try:
        got = ds.contains(p)
        assert got.inside.dtype == np.bool_ and got.crossings.shape == (p.shape[0], 3)
        assert got.inside[was_in].all() and was_in.sum() == 250
        sd = ds.signed_distance(p)
        assert (sd.distance[was_in] < 0).all() and np.array_equal(sd.inside, got.inside)
        ds.update(sc.ico_flat(offset=(0.0, 2.0 * sc.ICO_RADIUS, 0.0)))  # by its diameter
        got = ds.contains(p)
        assert not got.inside[was_in].any() and not got.votes[was_in].any()
        assert (ds.signed_distance(p).distance[was_in] > 0).all()
    finally:
        ds.close()


def test_a_split_clipped_handle_is_refused():
    flat = sc.scene("text_lowres")
    ds = DeviceScene(flat, 0, bvh={"split_depth": 3})
    try:
        refs = ds.bvh_info()["n_references"]
        assert refs > flat.n_triangles
        for call in (ds.contains, ds.signed_distance):
            with pytest.raises(_lib.RtError) as e:
                call(sc.points("text_lowres")[:8].copy())
            assert e.value.code == _abi.RT_ERR_UNSUPPORTED and "split clipping" in str(e.value) and str(refs) in str(e.value)
    finally:
        ds.close()


# torch is imported BEFORE librt_hip.so is loaded (a torch imported afterwards brings a second HIP runtime that finds no GPU):
# the test that hands tensors to the library runs in a child process of its own, as tests/test_ray_query_gpu.py's do
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch  # noqa: F401  (first)
import test_solid_gpu as T
T.{name}()
print("CHILD-OK")
"""


def test_torch_tensors_on_a_stream_and_closest_points_device():
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name="torch_tensors_on_a_stream")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def torch_tensors_on_a_stream():
    """(in the child process)"""
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for name in ("text_lowres", "solids"):
        flat, ds = _scene(name)
        p = sc.points(name)
        max_d = sc.max_distance(flat, p.shape[0])
        host = {(r, rule): (ds.contains(p, sc.table(r), rule), ds.signed_distance(p, max_d, sc.table(r), rule)) for r in (3, 8) for rule in sc.RULES}
        host_default = ds.signed_distance(p)
        near = ds.closest_points(p, max_d)
        tp, tm = torch.from_numpy(p).to(dev), torch.from_numpy(max_d).to(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            got = {(r, rule): (ds.contains(tp, sc.table(r), rule), ds.signed_distance(tp, tm, torch.from_numpy(sc.table(r)), rule)) for r in (3, 8)
                   for rule in sc.RULES}
            got_default = ds.signed_distance(tp)
            tnear = ds.closest_points(tp, tm)  # rt_closest_points_device on the same points
        stream.synchronize()
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a.cpu().numpy()).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))  # noqa: E731
        for key in host:
            (hc, hs), (gc, gs) = host[key], got[key]
            assert gc.inside.dtype == torch.bool and gc.votes.dtype == torch.uint8 and gc.crossings.dtype == torch.int32 and gc.inside.device == tp.device
            for f in hc._fields:
                assert same(getattr(gc, f), getattr(hc, f)), (name, key, "contains", f)
            for f in hs._fields:
                assert same(getattr(gs, f), getattr(hs, f)), (name, key, "signed_distance", f)
            # |sd| and every shared plane are rt_closest_points_device's
            assert torch.equal(gs.distance.abs().view(torch.int32), tnear.distance.view(torch.int32)), (name, key)
            for f in ("id", "point", "normal", "bary", "material"):
                assert torch.equal(getattr(gs, f), getattr(tnear, f)), (name, key, f)
            assert same(tnear.distance, near.distance)
            assert torch.equal(torch.signbit(gs.distance), gs.inside)
        for f in host_default._fields:
            assert same(getattr(got_default, f), getattr(host_default, f)), (name, "defaults", f)
        with pytest.raises(ValueError):
            ds.contains(tp, rule="odd")
        with pytest.raises(ValueError):
            ds.contains(tp, np.zeros((9, 3), F32))
        with pytest.raises(_lib.RtError):
            ds.contains(tp, np.zeros((1, 3), F32))
        ds.close()


def test_c_signed_distance_example_runs(tmp_path):
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "c_signed_distance_example"
    subprocess.check_call(["gcc", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_signed_distance_example.c"),
                           "-L", lib_dir, "-lrt_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device equals model: yes" in out.stdout and "model checksum" in out.stdout and "device checksum" in out.stdout
