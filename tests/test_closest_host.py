"""Closest-point queries on the CPU.  rt_closest_points_model (the specification: a linear scan with csrc/rt_closest.h) against
the independent float64 brute force of tests/f64_closest.py and against answers known by hand; misses, dead points and every
kind of search radius; rt_closest_packed (the KERNEL's walk -- seed descent, threaded walk, rt_closest_may_skip -- run on the
host over the packed blob) bit for bit against the model on every scene and four tree states, which is what shows that the
pruning never cuts a winner or a tie; and the validation errors.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_cases as cc
import f64_closest as f64
import scene_update_cases as upd
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

F32 = np.float32
ptr = lambda a: a.ctypes.data  # noqa: E731


# ---- the model against float64 ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def against_f64():
    """scene -> (flat, points, model planes, float64 minimum, float64 closest point / distance of the model's object, tol)"""
    cache = {}

    def get(name):
        if name not in cache:
            flat = cc.scene(name)
            pts = cc.points(flat, 2000, seed=11)
            m = cc.model(flat, pts)
            dmin, of = f64.brute(flat, pts)
            q64, d64 = of(m["id"])
            tol = cc.K * 2.0 ** -23 * f64.scale_of(flat, pts, m["id"])
            cache[name] = (flat, pts, m, dmin, q64, d64, tol)
        return cache[name]
    return get


@pytest.mark.parametrize("name", cc.SCENES)
def test_model_agrees_with_the_float64_brute_force(against_f64, name):
    flat, pts, m, dmin, q64, d64, tol = against_f64(name)
    hit = m["id"] >= 0
    fin = np.isfinite(pts).all(axis=1)
    assert np.array_equal(hit, fin & np.isfinite(dmin))  # a hit exactly where a finite point has a scene around it
    assert (~fin).sum() >= 4
    unit = tol / cc.K
    with np.errstate(invalid="ignore"):
        r_min = ((d64 - dmin) / unit)[hit]
        r_dist = (np.abs(m["distance"] - d64) / unit)[hit]
        r_point = (np.abs(m["point"].astype(np.float64) - q64).max(axis=1) / unit)[hit]
    print(name, "largest ratios to 2^-23 * scale: minimum %.3f distance %.3f point %.3f (K = %.2f)" % tuple(
        [float(r.max()) if r.size else 0.0 for r in (r_min, r_dist, r_point)] + [cc.K]))
    if not hit.any():
        return
    assert np.isfinite(m["distance"][hit]).all() and np.isfinite(m["point"][hit]).all() and np.isfinite(m["bary"][hit]).all()
    # the object the model chose is, in float64, within tol of the nearest (exact ties on shared edges are legitimate)
    assert (r_min <= cc.K).all(), float(r_min.max())
    assert (r_dist <= cc.K).all(), float(r_dist.max())
    assert (r_point <= cc.K).all(), float(r_point.max())
    # bary restates the point, and the material and normal are the object's
    tri = m["id"] >= flat.n_spheres
    t = m["id"][tri] - flat.n_spheres
    if tri.any():
        b = m["bary"][tri].astype(np.float64)
        q = flat.tri_v1[t] + b[:, :1] * flat.tri_e1[t] + b[:, 1:] * flat.tri_e2[t]
        assert (np.abs(q - m["point"][tri]).max(axis=1) <= tol[tri]).all()
        assert (b >= 0).all() and (b.sum(axis=1) <= 1 + 1e-6).all()
        assert np.array_equal(m["normal"][tri], flat.tri_normal[t]) and np.array_equal(m["material"][tri], flat.tri_material[t])
    sph = hit & ~tri
    if sph.any():
        assert np.array_equal(m["material"][sph], flat.sphere_material[m["id"][sph]]) and (m["bary"][sph] == 0).all()
        assert np.allclose(np.linalg.norm(m["normal"][sph], axis=1), 1.0, atol=1e-6)


def test_misses_and_dead_points_return_the_miss_values(against_f64):
    for name in ("empty", "test_scene"):
        flat, pts, m, *_ = against_f64(name)
        dead = m["id"] < 0
        assert dead.sum() >= 4
        assert (m["distance"][dead] == np.inf).all() and (m["material"][dead] == 0xFFFFFFFF).all()
        for plane in ("point", "normal", "bary"):
            assert (m[plane][dead].view(np.uint32) == 0).all(), plane
    assert (against_f64("empty")[2]["id"] == -1).all()


@pytest.mark.parametrize("name", ("test_scene", "degenerate", "text_lowres"))
def test_every_kind_of_radius(against_f64, name):
    flat, pts, free, *_ = against_f64(name)
    for kind in cc.RADII:
        r = cc.radii(flat, pts, kind, own_distance=free["distance"])
        m = cc.model(flat, pts, r)
        if kind in ("none", "inf", "own"):  # (own: the test is <=, the model's own distance still counts)
            assert cc.same_bits(m, free) == [], kind
        elif kind in ("negative", "nan"):
            assert (m["id"] == -1).all() and (m["distance"] == np.inf).all(), kind
        else:
            inside = (free["id"] >= 0) & (free["distance"] <= r)
            assert inside.any() and np.array_equal(m["id"] >= 0, inside), kind
            for plane, _, _ in cc.PLANES:
                assert np.array_equal(m[plane][inside], free[plane][inside]), (kind, plane)
            assert (m["distance"][~inside] == np.inf).all()
            if kind == "zero":
                assert (m["distance"][inside] == 0).all()


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_degenerate_scene():
    flat = cc.degenerate()
    q = [  # point, id, distance, closest point, bary (None: not checked)
        ((0.25, 0.25, -1.0), cc.DEG_PLAIN, 1.0, (0.25, 0.25, 0.0), (0.25, 0.25)),           # face region
        ((-1.0, -1.0, -1.0), cc.DEG_PLAIN, 3.0 ** 0.5, (0.0, 0.0, 0.0), (0.0, 0.0)),         # vertex region v1
        ((1.5, -1.0, 0.0), cc.DEG_PLAIN, 1.25 ** 0.5, (1.0, 0.0, 0.0), (1.0, 0.0)),          # vertex region v1 + e1
        ((0.5, -1.0, -1.0), cc.DEG_PLAIN, 2.0 ** 0.5, (0.5, 0.0, 0.0), (0.5, 0.0)),          # edge region e1
        ((-0.5, 0.5, -0.5), cc.DEG_PLAIN, 0.5 ** 0.5, (0.0, 0.5, 0.0), (0.0, 0.5)),          # edge region e2
        ((1.0, 1.0, -0.25), cc.DEG_PLAIN, (0.5 + 0.0625) ** 0.5, (0.5, 0.5, 0.0), (0.5, 0.5)),  # hypotenuse
        ((3.25, -1.0, 0.0), cc.DEG_SLIVER, 1.0, (3.25, 0.0, 0.0), (0.25, 0.0)),              # the sliver's long edge
        ((1.5, 4.0, 0.0), cc.DEG_COLLINEAR, 1.0, (1.5, 3.0, 0.0), None),                     # beyond the middle vertex: the longest segment
        ((0.25, 3.5, 0.0), cc.DEG_COLLINEAR, 0.5, (0.25, 3.0, 0.0), None),
        ((3.0, 2.0, 3.0), cc.DEG_POINT, 5.0 ** 0.5, (3.0, 3.0, 1.0), None),                  # nearer than the far end of the collinear one
        ((3.0, 3.0, 2.0), cc.DEG_POINT, 1.0, (3.0, 3.0, 1.0), None),                         # three equal vertices
        ((0.25, 0.25, 3.0), cc.DEG_TWIN_B, 1.0, (0.25, 0.25, 2.0), (0.25, 0.25)),            # coincident pair: the larger id
        ((5.0, 0.5, -1.0), cc.DEG_SHARE_B, 1.0, (5.0, 0.5, 0.0), None),                      # on the shared edge's side: equal distance, larger id
        ((0.25, 0.25, 0.5), cc.DEG_PLAIN, 0.5, (0.25, 0.25, 0.0), (0.25, 0.25)),             # the sphere's centre: sphere and triangle tie at r
        ((0.25, 0.25, 0.75), 0, 0.25, (0.25, 0.25, 1.0), (0.0, 0.0)),                        # inside the sphere: its surface, not its volume
        ((0.25, 0.25, 0.0), cc.DEG_PLAIN, 0.0, (0.25, 0.25, 0.0), (0.25, 0.25)),             # where the sphere touches the triangle: a tie at 0
    ]
    pts = np.array([x[0] for x in q], F32)
    m = cc.model(flat, pts)
    assert m["id"].tolist() == [x[1] for x in q]
    assert np.allclose(m["distance"], [x[2] for x in q], rtol=0, atol=1e-6)
    assert np.allclose(m["point"], [x[3] for x in q], rtol=0, atol=1e-6)
    for i, x in enumerate(q):
        if x[4] is not None:
            assert np.allclose(m["bary"][i], x[4], rtol=0, atol=1e-6), i
    for plane, _, _ in cc.PLANES:
        assert np.isfinite(m[plane].astype(np.float64)).all(), plane
    # a sphere's centre exactly: the direction is (1, 0, 0)
    ball = flat.without_triangles()
    c = cc.model(ball, ball.sphere_center[:1])
    assert c["id"][0] == 0 and c["distance"][0] == F32(0.5) and c["point"][0].tolist() == [0.75, 0.25, 0.5] and c["normal"][0].tolist() == [1.0, 0.0, 0.0]
    # every object of the scene, against a cloud of points: all results finite (no zero denominator anywhere)
    cloud = cc.points(flat, 4000, seed=3)[:-4]
    mm = cc.model(flat, cloud)
    assert (mm["id"] >= 0).all() and np.isfinite(mm["distance"]).all() and np.isfinite(mm["point"]).all() and np.isfinite(mm["bary"]).all()


# ---- the kernel's walk on the host ----------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime_api.h>
#include "rt_closest.h"
#include "rt_scene_pack.h"
static RtPackedScene g;
extern "C" {
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* counts) {
  const int rc = rt_pack_scene(d, budget, &g);
  counts[0] = g.dev.n_triangles, counts[1] = g.dev.n_slots, counts[2] = g.dev.n_nodes, counts[3] = g.dev.n_thr;
  return rc;
}
int probe_refit(const rt_scene_delta* d) { return rt_refit_packed(&g, d); }
int probe_rebuild(uint32_t* counts) {
  const int rc = rt_rebuild_packed(&g, 0);
  counts[0] = g.dev.n_triangles, counts[1] = g.dev.n_slots, counts[2] = g.dev.n_nodes, counts[3] = g.dev.n_thr;
  return rc;
}
void probe_closest(uint32_t n, const float* point, const float* max_distance, int32_t* id, float* distance, float* out_point, float* normal,
                   float* bary, uint32_t* material) {
  const RtClosestArgs a = {point, max_distance, id, distance, out_point, normal, bary, material, n};
  rt_closest_packed(g, a);
}
const char* probe_error() { return rt_last_error(); }
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("closest_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                   [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def packed(probe, pts, max_d):
    out = cc.new_planes(pts.shape[0])
    probe.probe_closest(C.c_uint32(pts.shape[0]), C.c_void_p(ptr(pts)), C.c_void_p(None if max_d is None else ptr(max_d)),
                        *[C.c_void_p(ptr(out[name])) for name, _, _ in cc.PLANES])
    return out


def pack(probe, flat, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    counts = np.zeros(4, np.uint32)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(_abi.RT_SCENE_BUDGET_DEFAULT), C.c_void_p(ptr(counts)))
    assert rc == 0, probe.probe_error()
    return [int(v) for v in counts]


@pytest.mark.parametrize("name", cc.SCENES)
def test_kernel_walk_equals_the_linear_scan_bit_for_bit(probe, name):
    flat = cc.scene(name)
    n = 5000 if name == "text" else 20000
    pts = cc.points(flat, n, seed=21)
    states = 0
    for with_radii in (False, True):
        r = cc.mixed_radii(flat, pts, seed=22) if with_radii else None
        want = cc.model(flat, pts, r)
        nt, n_slots, n_nodes, n_thr = pack(probe, flat)
        assert nt == flat.n_triangles
        assert cc.same_bits(packed(probe, pts, r), want) == [], ("packed", with_radii)
        states += 1
    if not flat.n_triangles:
        return
    # after a refit to a jittered mesh: the boxes are the refit's, the answer is the jittered description's
    moved = upd.jitter(flat, 0.05)
    delta, keep = _abi.make_scene_delta(moved, _abi.scene_delta_groups(flat, moved))
    assert probe.probe_refit(C.byref(delta)) == 0, probe.probe_error()
    r = cc.mixed_radii(moved, pts, seed=23)
    for rr in (None, r):
        assert cc.same_bits(packed(probe, pts, rr), cc.model(moved, pts, rr)) == [], "refitted"
    # after a rebuild: another tree, other slots, the same bits
    counts = np.zeros(4, np.uint32)
    assert probe.probe_rebuild(C.c_void_p(ptr(counts))) == 0, probe.probe_error()
    for rr in (None, r):
        assert cc.same_bits(packed(probe, pts, rr), cc.model(moved, pts, rr)) == [], "rebuilt"
    # split clipping: several references per triangle, each evaluates the whole triangle
    nt, n_slots, n_nodes, n_thr = pack(probe, flat, bvh={"split_depth": 3})
    if name in ("text_lowres", "text", "test_scene"):
        assert n_slots > nt, (n_slots, nt)
    r = cc.mixed_radii(flat, pts, seed=22)
    for rr in (None, r):
        assert cc.same_bits(packed(probe, pts, rr), cc.model(flat, pts, rr)) == [], "split"


def test_tree_shapes_without_a_walk(probe):
    """no triangles (n_thr == 0), and single roots: one triangle, and max_leaf triangles rebuilt into rt_lbvh_single_root"""
    base = cc.scene("test_scene")
    pts = cc.points(base, 2000, seed=31)
    for count in (0, 1, 2, 4):
        flat = upd.copy(base, tri_v1=base.tri_v1[:count], tri_e1=base.tri_e1[:count], tri_e2=base.tri_e2[:count], tri_normal=base.tri_normal[:count],
                        tri_material=base.tri_material[:count])
        nt, n_slots, n_nodes, n_thr = pack(probe, flat)
        assert nt == count and n_thr <= 2
        assert cc.same_bits(packed(probe, pts, None), cc.model(flat, pts)) == [], count
        if count:
            counts = np.zeros(4, np.uint32)
            assert probe.probe_rebuild(C.c_void_p(ptr(counts))) == 0, probe.probe_error()
            assert counts[3] == 1  # the single root
            assert cc.same_bits(packed(probe, pts, None), cc.model(flat, pts)) == [], ("rebuilt", count)


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    lib = _lib.load()
    flat = cc.scene("test_scene")
    desc, keep = _abi.make_scene_desc(flat)
    pts = cc.points(flat, 16, seed=1)
    out = cc.new_planes(16)
    b, h = cc.batch_struct(pts, None), cc.hits_struct(out)

    def refused(rc, word):
        assert rc == _abi.RT_ERR_INVALID_ARG, rc
        assert word in lib.rt_last_error().decode(), lib.rt_last_error()

    refused(lib.rt_closest_points_model(None, C.byref(b), C.byref(h)), "null scene")
    refused(lib.rt_closest_points(None, C.byref(b), C.byref(h)), "null scene")
    refused(lib.rt_closest_points_device(None, C.byref(b), C.byref(h), None), "null scene")
    refused(lib.rt_closest_points_model(C.byref(desc), None, C.byref(h)), "null point batch")
    refused(lib.rt_closest_points_model(C.byref(desc), C.byref(b), None), "null output")
    bad = cc.batch_struct(pts, None)
    bad.abi_version = _abi.RT_ABI_VERSION + 1
    refused(lib.rt_closest_points_model(C.byref(desc), C.byref(bad), C.byref(h)), "abi_version")
    bad = cc.batch_struct(pts, None)
    bad.point = None
    refused(lib.rt_closest_points_model(C.byref(desc), C.byref(bad), C.byref(h)), "point missing")
    refused(lib.rt_closest_points_model(C.byref(desc), C.byref(b), C.byref(_abi.rt_point_hits())), "every output plane")
    # n_points == 0 is a no-op, with or without arrays; a single plane is enough
    empty = _abi.rt_point_batch(_abi.RT_ABI_VERSION, 0, None, None)
    assert lib.rt_closest_points_model(C.byref(desc), C.byref(empty), C.byref(h)) == 0
    one = _abi.rt_point_hits()
    one.distance = out["distance"].ctypes.data
    assert lib.rt_closest_points_model(C.byref(desc), C.byref(b), C.byref(one)) == 0
    assert np.array_equal(out["distance"], cc.model(flat, pts)["distance"]) and (out["id"] == 0).all()
