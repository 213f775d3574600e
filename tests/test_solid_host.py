"""Containment and signed-distance queries on the CPU.  rt_contains_points_model / rt_signed_distance_model (the specification: a
linear scan with csrc/rt_solid.h) against answers known by hand, against rt_list_intersections_model's `total` ray by ray,
against float64 truth derived from the meshes (an icosphere's inradius; a brute-force Moeller-Trumbore parity written here) and
against rt_closest_points_model bit for bit; rt_solid_packed (the KERNEL's walk run on the host over the packed blob) bit for bit
against the model on blobs packed plain, refitted and rebuilt (LBVH and PLOC), and refused on a split-clipped one; the open mesh's
diagnostic; and the validation errors.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_cases as cc
import f64_closest
import multi_hit_cases as mh
import scene_update_cases as upd
import solid_cases as sc
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib, sampling
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

F32 = np.float32
ptr = sc.ptr

# ---- the kernel's walk on the host ----------------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime_api.h>
#include "rt_closest.h"
#include "rt_solid.h"
#include "rt_scene_pack.h"
static RtPackedScene g;
extern "C" {
static void counts_of(uint32_t* counts) { counts[0] = g.dev.n_triangles, counts[1] = g.dev.n_slots, counts[2] = g.dev.n_nodes, counts[3] = g.dev.n_thr; }
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* counts) {
  const int rc = rt_pack_scene(d, budget, &g);
  counts_of(counts);
  return rc;
}
int probe_refit(const rt_scene_delta* d) { return rt_refit_packed(&g, d); }
int probe_rebuild(uint32_t ploc, uint32_t* counts) {
  const int rc = ploc ? rt_rebuild_ploc_packed(&g, 0, 0) : rt_rebuild_packed(&g, 0);
  counts_of(counts);
  return rc;
}
// the two kernels of a signed-distance call in their order: the closest-point walk, then the containment walk on its distances
int probe_solid(uint32_t n, uint32_t n_dirs, uint32_t rule, const float* point, const float* max_distance, const float* dirs, float* signed_distance,
                uint8_t* inside, uint8_t* votes, uint32_t* crossings, int32_t* winding, int32_t* id, float* distance, float* out_point, float* normal,
                float* bary, uint32_t* material) {
  RtClosestArgs ca = {point, max_distance, id, distance, out_point, normal, bary, material, n};
  RtSolidArgs sa = {};
  sa.point = point, sa.inside = inside, sa.votes = votes, sa.crossings = crossings, sa.winding = winding, sa.signed_distance = signed_distance;
  sa.n = n, sa.n_dirs = n_dirs, sa.rule = rule;
  for (uint32_t r = 0; r < n_dirs; r++)
    for (int k = 0; k < 3; k++) sa.dir[r][k] = dirs[3 * r + k];
  if (rt_check_solid(g.dev, "probe_solid") != RT_OK) return RT_ERR_UNSUPPORTED;
  if (signed_distance) {
    if (!ca.distance) ca.distance = signed_distance;
    sa.distance = ca.distance;
  }
  if (ca.id || ca.distance || ca.out_point || ca.normal || ca.bary || ca.material) rt_closest_packed(g, ca);
  return rt_solid_packed(g, sa);
}
const char* probe_error() { return rt_last_error(); }
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("solid_probe")
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


def packed(probe, p, dirs, rule="parity", max_d=None, names=sc.SD_PLANES, expect=0):
    out = sc.new_planes(p.shape[0], dirs.shape[0], names, fill=0xA5)
    rc = probe.probe_solid(C.c_uint32(p.shape[0]), C.c_uint32(dirs.shape[0]), C.c_uint32(sc.RULE[rule]), C.c_void_p(ptr(p)), C.c_void_p(ptr(max_d)),
                           C.c_void_p(ptr(dirs)), *[C.c_void_p(ptr(out[name]) if name in out else None) for name in sc.SD_PLANES])
    assert rc == expect, probe.probe_error()
    return out


def pack(probe, flat, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    counts = np.zeros(4, np.uint32)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(_abi.RT_SCENE_BUDGET_DEFAULT), C.c_void_p(ptr(counts)))
    assert rc == 0, probe.probe_error()
    return [int(v) for v in counts]


def both(probe, flat):
    """-> the two implementations as call(p, dirs, rule) -> planes of a signed-distance call"""
    pack(probe, flat)
    return (lambda p, dirs, rule="parity": sc.sd_model(flat, p, dirs, rule)), (lambda p, dirs, rule="parity": packed(probe, p, dirs, rule))


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------------
def test_default_table_and_grid():
    t = sampling.solid_directions()
    assert t.dtype == F32 and np.array_equal(t, np.array([(1, 2, 3), (2, -3, 1), (-3, -1, 2)], F32))
    u = t.astype(np.float64) / np.linalg.norm(t.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(u @ u.T - np.eye(3)).max() < 0.08  # pairwise near-orthogonal
    # none is parallel to an axis or to a face diagonal: every component is non-zero and no two have the same magnitude
    a = np.abs(t)
    assert (a > 0).all() and all(len(set(row)) == 3 for row in a.tolist())
    g = sampling.grid_points((0, 1, 2), (1, 3, 2), (3, 2, 1))
    assert g.dtype == F32 and g.shape == (6, 3)
    assert np.array_equal(g, np.array([(0, 1, 2), (0, 3, 2), (0.5, 1, 2), (0.5, 3, 2), (1, 1, 2), (1, 3, 2)], F32))


def test_known_answers(probe):
    flat = sc.scene("solids")
    p = np.array([sc.SLAB_CENTRE, sc.OVERLAP_POINT, sc.NESTED_POINT, sc.FAR_POINT], F32)
    for r in sc.TABLES:
        dirs = sc.table(r)
        for call in both(probe, flat):
            par, win = call(p, dirs, "parity"), call(p, dirs, "winding")
            # (row 3 of the R = 8 table is (0, 0, 1): from the slab's centre it leaves exactly through the diagonal of the top face,
            # the case the default table is built to avoid; the other seven rows outvote whatever it counts)
            rows = [k for k in range(r) if not (r == 8 and k == 3)]
            for got in (par, win):
                # the slab centre: inside, one crossing per direction, and it leaves; half the smallest side, to the bit
                # (a row of the R = 8 table goes on through slab 1: three crossings, two of them leaving)
                assert got["inside"][0] == 1 and got["votes"][0] >= len(rows) and (got["crossings"][0, rows] % 2 == 1).all()
                assert (got["winding"][0, rows] == 1).all() and (r == 8 or (got["crossings"][0] == 1).all())
                assert got["signed_distance"][0] == F32(-0.5) and got["distance"][0] == F32(0.5)
                # far away: all zero
                assert got["inside"][3] == 0 and got["votes"][3] == 0 and not got["crossings"][3].any() and not got["winding"][3].any()
                assert got["signed_distance"][3] > 0 and got["signed_distance"][3] == got["distance"][3]
                # the overlap of two slabs: every ray leaves two surfaces
                assert (got["crossings"][1] == 2).all() and (got["winding"][1] == 2).all()
                # the centre of the inner sphere: no triangle in any direction here or there, two spheres contain it
                assert not got["winding"][2].any() and (got["crossings"][2] % 2 == 0).all()
            # ... which pins the difference between the rules
            assert par["inside"][1] == 0 and par["votes"][1] == 0 and win["inside"][1] == 1 and win["votes"][1] == r
            assert par["inside"][2] == 0 and par["votes"][2] == 0 and win["inside"][2] == 1 and win["votes"][2] == r
            assert par["signed_distance"][2] == F32(0.25) and win["signed_distance"][2] == F32(-0.25)
    # the centre of a single sphere: -r
    base = mh.scene("test_scene")
    z3, zu = np.zeros((0, 3), F32), np.zeros((0,), np.uint32)
    ball = FlatScene(np.array([(1, 2, 3)], F32), np.array([4.0], F32), np.array([0.5], F32), np.array([0], np.uint32), z3, z3, z3, z3, zu,
                     base.materials, base.lights).contiguous()
    q = np.array([(1, 2, 3), (1, 2, 4.5), (1, 2, 5.5), (1, 2, 5)], F32)
    for call in both(probe, ball):
        for rule in sc.RULES:
            got = call(q, sc.table(3), rule)
            assert got["signed_distance"].tolist() == [-2.0, -0.5, 0.5, 0.0] and got["inside"].tolist() == [1, 1, 0, 0]  # (on the surface: cc == 0 is outside)
            assert got["votes"].tolist() == [3, 3, 0, 0]
    # a NaN and a negative r_sq never contain
    for r_sq in (np.nan, -4.0):
        bad = FlatScene(ball.sphere_center, np.array([r_sq], F32), ball.sphere_r_inv, ball.sphere_material, z3, z3, z3, z3, zu, base.materials, base.lights)
        desc, keep = _abi.make_scene_desc(bad.contiguous())
        out = sc.new_planes(4, 3, sc.SOLID_PLANES)
        rc = _lib.load().rt_contains_points_model(C.byref(desc), C.byref(sc.batch_struct(q, sc.table(3))), C.byref(sc.solid_struct(out)))
        if rc == 0:  # (a description check may refuse such a radius; where it passes, nothing is inside)
            assert not out["inside"].any() and not out["votes"].any()


# ---- 2. crossings against the multi-hit specification ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SCENES)
def test_crossings_equal_the_total_of_list_intersections(name):
    flat = sc.triangles_only(sc.scene(name))
    p = sc.points(name)
    n = p.shape[0]
    for r in sc.TABLES:
        dirs = sc.table(r)
        got = sc.contains_model(flat, p, dirs)
        o = np.ascontiguousarray(np.repeat(p, r, axis=0))
        d = np.ascontiguousarray(np.tile(dirs, (n, 1)))
        total = mh.model(flat, o, d, 16, None, cull=False, total=True)["total"].reshape(n, r)
        assert np.array_equal(got["crossings"], total), (name, r)
        assert not got["crossings"][sc.DEAD].any() and not got["winding"][sc.DEAD].any()
        assert not got["inside"][sc.DEAD].any() and not got["votes"][sc.DEAD].any()
        assert (np.abs(got["winding"]) <= got["crossings"]).all()
        # without spheres the vote is the crossings' parity
        assert np.array_equal(got["votes"], (got["crossings"] & 1).sum(axis=1).astype(np.uint8))
        assert np.array_equal(got["inside"], (2 * got["votes"].astype(int) > r).astype(np.uint8))


# ---- 3. float64 truth ---------------------------------------------------------------------------------------------------------------------
def ico_points(n=500, seed=31):
    """half within 0.9 inradii of the centre, half between 1.1 and 4 radii from it; float32, and the float64 |p - c| of the cast points"""
    rng = np.random.default_rng(seed)
    c, r, r_in = np.array(sc.ICO_CENTRE), sc.ICO_RADIUS, sc.ico_inradius()
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.where(np.arange(n) < n // 2, 0.9 * r_in * rng.random(n) ** (1 / 3), r * rng.uniform(1.1, 4.0, n))
    p = (c + u * rad[:, None]).astype(F32)
    cs, rs = sc.ICO_SPHERE
    p[-10:] = (np.array(cs) + u[-10:] * (0.8 * rs * rng.random(10))[:, None]).astype(F32)  # ten points inside the sphere beside it
    return p, np.linalg.norm(p.astype(np.float64) - c, axis=1)


def test_ico_inside_equals_the_analytic_answer():
    flat = sc.scene("ico")
    r, r_in = sc.ICO_RADIUS, sc.ico_inradius()
    assert 0.99 * r < r_in < r
    p, dist = ico_points()
    # (the cast to float32 moves a point by 1e-7: the two shells keep a margin of a thousand times that)
    in_ico = dist <= 0.9 * r_in + 1e-6
    assert (in_ico | (dist >= 1.1 * r - 1e-6)).all() and in_ico.sum() == 250
    cs, rs = np.array(sc.ICO_SPHERE[0]), sc.ICO_SPHERE[1]
    ds = np.linalg.norm(p.astype(np.float64) - cs, axis=1)
    assert (np.abs(ds - rs) > 1e-4).all() and (ds < rs).any()
    want = in_ico | (ds < rs)
    for rule in sc.RULES:
        for t in sc.TABLES:
            got = sc.sd_model(flat, p, sc.table(t), rule)
            assert np.array_equal(got["inside"].astype(bool), want), (rule, t)
            assert ((got["votes"] == 0) | (got["votes"] == t)).all(), (rule, t)
            depth = -got["signed_distance"][in_ico].astype(np.float64)
            assert (depth >= r_in - dist[in_ico] - 1e-5).all() and (depth <= r - dist[in_ico] + 1e-5).all(), (rule, t)


def moeller_trumbore_parity(flat, p, dirs):
    """float64 brute force -> crossings (n, R): Moeller-Trumbore (not the matrix inverse of the library) on every triangle"""
    v1, e1, e2 = (a.astype(np.float64) for a in (flat.tri_v1, flat.tri_e1, flat.tri_e2))
    P = p.astype(np.float64)
    out = np.zeros((p.shape[0], dirs.shape[0]), np.int64)
    for r, d in enumerate(dirs.astype(np.float64)):
        d = d / np.linalg.norm(d)
        h = np.cross(d, e2)                        # (T, 3)
        a = np.einsum("tk,tk->t", e1, h)
        ok = np.abs(a) > 1e-12
        f = 1.0 / np.where(ok, a, 1.0)
        s = P[:, None, :] - v1[None]               # (n, T, 3)
        u = f * np.einsum("ntk,tk->nt", s, h)
        q = np.cross(s, e1[None])
        v = f * np.einsum("ntk,k->nt", q, d)
        t = f * np.einsum("ntk,tk->nt", q, e2)
        out[:, r] = (ok[None] & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)).sum(axis=1)
    return out


def test_solids_inside_equals_a_float64_parity():
    flat = sc.scene("solids")
    p = sc.points("solids")[sc.FREE]
    keep = f64_closest.brute(flat, p)[0] > 1e-4 * sc.extent(flat)
    assert keep.mean() >= 0.99, keep.mean()  # at most 1 % of the points may lie that close to a surface
    c, r_sq = flat.sphere_center.astype(np.float64), flat.sphere_r_sq.astype(np.float64)
    k_s = ((np.linalg.norm(p.astype(np.float64)[:, None] - c[None], axis=2) ** 2 - r_sq[None]) < 0).sum(axis=1)
    for t in sc.TABLES:
        dirs = sc.table(t)
        vote = ((moeller_trumbore_parity(flat, p, dirs) + k_s[:, None]) & 1).astype(bool)
        # the condition the seed of the point set was picked for: the float64 model alone is unanimous on every kept point
        assert (vote[keep].all(axis=1) | ~vote[keep].any(axis=1)).all(), t
        got = sc.contains_model(flat, sc.points("solids"), dirs, "parity")
        assert np.array_equal(got["inside"][sc.FREE][keep].astype(bool), vote[keep, 0]), t
    assert 0.02 < vote[keep, 0].mean() < 0.5  # both answers occur


# ---- 4. the distance is rt_closest_points' ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_max_d", (False, True))
@pytest.mark.parametrize("name", sc.SCENES)
def test_distance_planes_have_the_bits_of_closest_points(name, with_max_d):
    flat, p = sc.scene(name), sc.points(name)
    max_d = sc.max_distance(flat, p.shape[0]) if with_max_d else None
    want = cc.model(flat, p, max_d)
    for rule in sc.RULES:
        got = sc.cached_sd_model(name, 3, rule, with_max_d)
        assert cc.same_bits(got, want) == [], (name, rule)
        mag = np.abs(got["signed_distance"])
        assert np.array_equal(mag.view(np.uint32), want["distance"].view(np.uint32))
        neg = np.signbit(got["signed_distance"])
        assert np.array_equal(neg, got["inside"].astype(bool))  # (a distance of 0 inside is -0)
        # the containment planes do not depend on the radius
        assert sc.same_bits({k: got[k] for k in sc.SOLID_PLANES}, sc.contains_model(flat, p, sc.table(3), rule)) == []
    if with_max_d and name != "empty":
        miss = want["id"] < 0
        assert miss[:-sc.N_DEAD].any() and np.isinf(got["signed_distance"][miss]).all()


# ---- 5. the open mesh ----------------------------------------------------------------------------------------------------------------------
def test_open_mesh_shows_as_disagreeing_directions():
    """text_lowres is an open surface (561 boundary edges of 2 739).  Of its 486 free points 20 are non-unanimous at the default
    R = 3 and 28 at R = 8 (parity): the diagnostic the definition gives an open mesh instead of a refusal.  The closed scenes
    have none among their free points."""
    for r in (3, 8):
        v = sc.cached_sd_model("text_lowres", r, "parity")["votes"][sc.FREE]
        count = int(((v != 0) & (v != r)).sum())
        print("text_lowres R = %d: %d of %d free points non-unanimous" % (r, count, v.size))
        assert count > 0
    for name in ("ico", "spheres", "empty"):
        v = sc.cached_sd_model(name, 3, "parity")["votes"][sc.FREE]
        assert ((v == 0) | (v == 3)).all(), name


# ---- 6. the kernel's walk on the host ------------------------------------------------------------------------------------------------------
def twin_equals_model(probe, flat, name, state):
    p = sc.points(name)
    for r, rule, with_max_d in ((1, "parity", False), (3, "parity", True), (3, "winding", False), (8, "parity", False), (8, "winding", True)):
        max_d = sc.max_distance(flat, p.shape[0]) if with_max_d else None
        want = sc.sd_model(flat, p, sc.table(r), rule, max_d)
        got = packed(probe, p, sc.table(r), rule, max_d)
        assert sc.same_bits(got, want) == [], (name, state, r, rule, with_max_d)


@pytest.mark.parametrize("name", sc.SCENES)
def test_kernel_walk_equals_the_linear_scan_bit_for_bit(probe, name):
    flat = sc.scene(name)
    nt, n_slots, n_nodes, n_thr = pack(probe, flat)
    assert nt == flat.n_triangles == n_slots
    if name in ("ico", "text_lowres"):
        assert n_thr > 100  # a tree of real depth
    twin_equals_model(probe, flat, name, "packed")
    if not flat.n_triangles:
        return
    # after a refit to a jittered mesh: the boxes are the refit's, the answer is the jittered description's
    moved = upd.jitter(flat, 0.05)
    delta, keep = _abi.make_scene_delta(moved, _abi.scene_delta_groups(flat, moved))
    assert probe.probe_refit(C.byref(delta)) == 0, probe.probe_error()
    twin_equals_model(probe, moved, name, "refitted")
    # after a rebuild, LBVH then PLOC: other trees, other slots, the same bits
    counts = np.zeros(4, np.uint32)
    for ploc in (0, 1):
        assert probe.probe_rebuild(C.c_uint32(ploc), C.c_void_p(ptr(counts))) == 0, probe.probe_error()
        twin_equals_model(probe, moved, name, "rebuilt, ploc %d" % ploc)


def test_split_clipped_trees_are_refused(probe):
    flat = sc.scene("text_lowres")
    nt, n_slots, _, _ = pack(probe, flat, bvh={"split_depth": 3})
    assert n_slots > nt
    p = sc.points("text_lowres")[:16].copy()
    out = packed(probe, p, sc.table(3), expect=_abi.RT_ERR_UNSUPPORTED)
    msg = probe.probe_error().decode()
    assert "split clipping" in msg and str(n_slots) in msg and str(nt) in msg, msg
    for a in out.values():
        assert (a.view(np.uint8) == 0xA5).all()  # nothing was written


def test_null_planes_of_the_twin_are_not_written(probe):
    flat = sc.scene("ico")
    pack(probe, flat)
    p = sc.points("ico")[-70:].copy()
    want = sc.sd_model(flat, p, sc.table(3))
    for names in (("inside",), ("votes", "winding"), ("crossings",), ("signed_distance",), ("signed_distance", "distance", "id")):
        got = packed(probe, p, sc.table(3), names=names)
        assert sc.same_bits(got, {k: want[k] for k in names}) == [], names


# ---- 7. validation --------------------------------------------------------------------------------------------------------------------------
def test_validation_errors_and_null_planes():
    lib = _lib.load()
    flat = sc.scene("solids")
    desc, keep = _abi.make_scene_desc(flat)
    p = sc.points("solids")[:16].copy()
    dirs = sc.table(3)
    out = sc.new_planes(16, 3, fill=0xA5)
    untouched = {name: a.copy() for name, a in out.items()}
    so, sd = sc.solid_struct(out), sc.sd_struct(out)
    good = lambda **kw: sc.batch_struct(p, kw.pop("dirs", dirs), **kw)  # noqa: E731

    def refused(rc, word):
        assert rc == _abi.RT_ERR_INVALID_ARG, rc
        assert word in lib.rt_last_error().decode(), lib.rt_last_error()
        assert sc.same_bits(out, untouched) == []  # nothing was written

    def every_call(b, word):
        refused(lib.rt_contains_points_model(C.byref(desc), C.byref(b), C.byref(so)), word)
        refused(lib.rt_signed_distance_model(C.byref(desc), C.byref(b), C.byref(sd)), word)

    for fn, o in ((lib.rt_contains_points_model, so), (lib.rt_signed_distance_model, sd)):
        refused(fn(None, C.byref(good()), C.byref(o)), "null scene")
        refused(fn(C.byref(desc), None, C.byref(o)), "null solid batch")
        refused(fn(C.byref(desc), C.byref(good()), None), "null output")
    for fn, o in ((lib.rt_contains_points, so), (lib.rt_signed_distance, sd)):
        refused(fn(None, C.byref(good()), C.byref(o)), "null scene")
    for fn, o in ((lib.rt_contains_points_device, so), (lib.rt_signed_distance_device, sd)):
        refused(fn(None, C.byref(good()), C.byref(o), None), "null scene")
    bad = good()
    bad.abi_version = _abi.RT_ABI_VERSION + 1
    every_call(bad, "abi_version")
    bad = good()
    bad.point = None
    every_call(bad, "point missing")
    bad = good()
    bad.directions = None
    every_call(bad, "directions missing")
    nine = np.ascontiguousarray(np.tile(dirs, (3, 1)))
    for wrong in (0, 9, 0xFFFFFFFF):  # R = 0 and R = 9
        bad = good(dirs=nine)
        bad.n_directions = wrong
        every_call(bad, "n_directions")
    for row in ((0, 0, 0), (np.nan, 1, 0), (1, np.inf, 0), (1e-30, 0, 0), (3e38, 3e38, 0)):  # zero, NaN, inf; |d|^2 under- and overflows
        t = dirs.copy()
        t[1] = row
        every_call(good(dirs=t), "direction 1")
    for wrong in (2, 0xFFFFFFFF):
        every_call(good(rule=wrong), "unknown rule")
    refused(lib.rt_contains_points_model(C.byref(desc), C.byref(good()), C.byref(_abi.rt_solid_out())), "every output plane")
    refused(lib.rt_signed_distance_model(C.byref(desc), C.byref(good()), C.byref(_abi.rt_signed_distance_out())), "every output plane")
    # n_points == 0 is a no-op, with or without arrays
    empty = _abi.rt_solid_batch(_abi.RT_ABI_VERSION, 0, None, None, 3, 0, ptr(dirs))
    assert lib.rt_contains_points_model(C.byref(desc), C.byref(empty), C.byref(so)) == 0
    assert lib.rt_signed_distance_model(C.byref(desc), C.byref(empty), C.byref(sd)) == 0
    assert sc.same_bits(out, untouched) == []
    # a NULL plane is not written, the others are: one plane at a time, each between guard words
    max_d = sc.max_distance(flat, 16)
    want = sc.sd_model(flat, p, dirs, "winding", max_d)
    for name in want:
        guarded = {m: np.full((a.nbytes + 3) // 4 + 8, 0x5A5A5A5A, np.uint32) for m, a in want.items()}
        views = {m: guarded[m][4:-4].view(np.uint8)[:want[m].nbytes].view(want[m].dtype).reshape(want[m].shape) for m in want}
        b = good(rule="winding", max_d=max_d)
        assert lib.rt_signed_distance_model(C.byref(desc), C.byref(b), C.byref(sc.sd_struct(views, only=(name,)))) == 0, lib.rt_last_error()
        if name in sc.SOLID_PLANES:
            b = good(rule="winding")
            assert lib.rt_contains_points_model(C.byref(desc), C.byref(b), C.byref(sc.solid_struct(views, only=(name,)))) == 0, lib.rt_last_error()
        for m in want:
            assert (guarded[m][:4] == 0x5A5A5A5A).all() and (guarded[m][-4:] == 0x5A5A5A5A).all(), (name, m)
            if m == name:
                assert np.array_equal(views[m].view(np.uint8), want[m].view(np.uint8)), name
            else:
                assert (guarded[m] == 0x5A5A5A5A).all(), (name, m)


def test_header_and_exports():
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "#define RT_ABI_VERSION 4u" in text  # additive: the version stays
    assert "#define RT_MAX_SOLID_DIRECTIONS 8u" in text and _abi.RT_MAX_SOLID_DIRECTIONS == 8
    for name in ("rt_contains_points", "rt_contains_points_device", "rt_contains_points_model", "rt_signed_distance", "rt_signed_distance_device",
                 "rt_signed_distance_model"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in text, name
    csrc = lambda f: open(os.path.join(CSRC, f)).read()  # noqa: E731
    assert "rt_solid.h" in csrc("rt_closest.h") and "rt_solid.h" in csrc("rt_multihit.h")  # the two gaps point to their answer
    assert "RT_ERR_UNSUPPORTED" in csrc("rt_solid.h")
