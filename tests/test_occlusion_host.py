"""Ambient-occlusion queries on the CPU.  The frame, origin and table rows of rt_occlusion_rays_model against a float64 numpy
restatement; the per-sample bit of rt_ambient_occlusion_model (the specification: a linear scan with csrc/rt_occlusion.h) against
three independent references on the model's own rays -- the oracle's has_any_intersection, its completely_occluded, and
rt_list_intersections_model at K = 1; the reductions against a numpy recomputation from the model's bits and rays;
rt_occlusion_packed (the KERNEL's walk run on the host over the packed blob) bit for bit against the model on blobs packed plain,
split-clipped, refitted and rebuilt (LBVH and PLOC); answers known by hand; the validation errors; and the condition that the
point sets are not degenerate.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import multi_hit_cases as mh
import occlusion_cases as oc
import ray_query_cases as rq
import scene_update_cases as upd
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

F32 = np.float32
ptr = oc.ptr
IDENTITY = np.eye(3, dtype=F32)  # a table whose three rows give tx, ty and n themselves: fma(1, tx, fma(0, ty, 0 * n)) = tx


# ---- 1. frame, origin, rows ---------------------------------------------------------------------------------------------------
def frame64(nrm):
    """Duff et al. 2017 in float64 on the float64 unit normal -> tx, ty, n"""
    n = nrm.astype(np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    sg = np.copysign(1.0, n[:, 2])
    a = -1.0 / (sg + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    tx = np.stack([1.0 + sg * n[:, 0] * n[:, 0] * a, sg * b, -sg * n[:, 0]], axis=1)
    ty = np.stack([b, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    return tx, ty, n


@pytest.mark.parametrize("bias", oc.BIASES)
@pytest.mark.parametrize("name", ("test_scene", "empty"))
def test_frame_origin_and_rows_of_the_rays_model(name, bias):
    p, nrm = oc.points(name)
    live = slice(0, p.shape[0] - oc.N_DEAD)
    o, basis, alive = oc.rays_model(p, nrm, 3, IDENTITY, bias=bias)
    assert alive[live].all() and not alive[-oc.N_DEAD:].any()
    tx, ty, n = basis[live, 0], basis[live, 1], basis[live, 2]
    # the frame against float64: each component is at most five rounded operations, within 1e-6 (about 8 ulp of 1)
    tx64, ty64, n64 = frame64(nrm[live])
    for got, want in ((tx, tx64), (ty, ty64), (n, n64)):
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-6
    g = np.stack([tx, ty, n], axis=1).astype(np.float64)
    assert np.abs(np.einsum("nik,njk->nij", g, g) - np.eye(3)).max() <= 1e-6  # orthonormal
    assert np.abs(np.cross(g[:, 0], g[:, 1]) - g[:, 2]).max() <= 2e-6  # right-handed: tx x ty = n
    # the normal and the origin are the definition's operations exactly
    # (compared as values: a component -0 of the frame comes through the identity table as fma(0, tx, fma(0, ty, -0)) = +0)
    n32 = oc.normalize32(nrm[live])
    assert np.array_equal(n, n32)
    assert np.array_equal(o[live].view(np.uint32), oc.fma32(n32, F32(bias), p[live]).view(np.uint32))
    # the rows wrap exactly, and the world direction is the three fused operations on them
    s, tab, first = 65, oc.table(), oc.first(p.shape[0])
    for f in (first, None):
        _, w, _ = oc.rays_model(p, nrm, s, tab, f, bias)
        l = tab[oc.rows(f, s, tab.shape[0])]  # (n or 1, S, 3)
        l = np.broadcast_to(l, (p.shape[0], s, 3))[live]
        want = oc.fma32(l[..., 0:1], tx[:, None, :], oc.fma32(l[..., 1:2], ty[:, None, :], l[..., 2:3] * n[:, None, :]))
        assert np.array_equal(w[live], want)
        # u against the float64 direction
        u = oc.normalize32(w[live]).astype(np.float64)
        l64 = l.astype(np.float64)
        d64 = l64[..., 0:1] * tx64[:, None, :] + l64[..., 1:2] * ty64[:, None, :] + l64[..., 2:3] * n64[:, None, :]
        ok = np.linalg.norm(d64, axis=2) > 0  # (the zero row of the table has no direction)
        d64 = d64 / np.where(ok, np.linalg.norm(d64, axis=2), 1.0)[..., None]
        assert np.abs(u - d64)[ok].max() <= 1e-6
        assert np.isnan(u[~ok]).all() and (~ok).any()


# ---- 2. independent references ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def any_ref(tmp_path_factory):
    return rq.build_ref(tmp_path_factory.mktemp("occlusion_ref"))


def dead_rays(o, w, alive):
    """(n, S): rays the definition counts as occluded without casting them"""
    with np.errstate(all="ignore"):
        u = oc.normalize32(w)
    return ~alive[:, None] | np.isnan(u).any(axis=2) | ~np.isfinite(o).all(axis=1)[:, None]


@pytest.mark.parametrize("kind", ("inf", "fraction"))
@pytest.mark.parametrize("name", oc.SCENES)
def test_bits_equal_three_independent_references(any_ref, name, kind):
    flat = oc.scene(name)
    p, nrm = oc.points(name)
    s, tab, first, bias = 64, oc.table(), oc.first(p.shape[0]), 1e-4
    max_d = oc.max_distance(kind, flat)
    o, w, alive = oc.rays_model(p, nrm, s, tab, first, bias)
    dead = dead_rays(o, w, alive)
    assert dead[-oc.N_DEAD:].all() and dead[:-oc.N_DEAD].any() and not dead[:-oc.N_DEAD].all(axis=1).any()
    ro, rd = np.ascontiguousarray(np.repeat(o, s, axis=0)), np.ascontiguousarray(w.reshape(-1, 3))
    rm = np.full(ro.shape[0], max_d, F32)
    live = ~dead.ravel()
    # (the references get a harmless ray in place of a dead one)
    ro[~live], rd[~live] = 0.0, (0.0, 0.0, 1.0)
    ref = rq.ref_any(any_ref, flat, ro, rd, rm)
    lists = mh.model(flat, ro, rd, 1, rm, total=False)
    plain = oc.unpack(oc.cached_model(name, s, kind=kind)["bits"], s).ravel()
    passed = oc.unpack(oc.cached_model(name, s, kind=kind, pass_transmissive=True)["bits"], s).ravel()
    assert plain[~live].all() and passed[~live].all()
    assert np.array_equal(plain[live], ref["has_intersection"].astype(bool)[live])
    assert np.array_equal(plain[live], (lists["count"] > 0)[live])
    assert np.array_equal(passed[live], ref["completely_occluded"].astype(bool)[live])
    assert not (passed & ~plain).any()


# ---- 3. reductions ---------------------------------------------------------------------------------------------------------------
def check_reductions(name, s, **kw):
    p, nrm = oc.points(name)
    got = oc.cached_model(name, s, **kw)
    o, w, alive = oc.rays_model(p, nrm, s, oc.table(), oc.first(p.shape[0]) if kw.get("first_on", True) else None, kw.get("bias", 1e-4))
    with np.errstate(all="ignore"):
        u = oc.normalize32(w)
    want = oc.reductions(oc.unpack(got["bits"], s), u, s)
    assert oc.same_bits(got, want) == [], (name, s, kw)
    # dead points: bits all set (the unused high bits 0), clear 0, visibility 0, bent normal 0
    full = oc.reductions(np.ones((1, s), bool), np.zeros((1, s, 3), F32), s)["bits"][0]
    dead = slice(-oc.N_DEAD, None)
    assert (got["bits"][dead] == full).all() and (got["clear"][dead] == 0).all()
    assert (got["visibility"][dead].view(np.uint32) == 0).all() and (got["bent_normal"][dead].view(np.uint32) == 0).all()
    return got


@pytest.mark.parametrize("s", oc.S_LIST)
def test_reductions_equal_a_numpy_recomputation_at_every_sample_count(s):
    got = check_reductions("test_scene", s)
    assert got["clear"].max() <= s
    check_reductions("test_scene", s, first_on=False, bias=0.0, kind="fraction", pass_transmissive=True)


@pytest.mark.parametrize("kind", oc.MAX_D)
@pytest.mark.parametrize("name", oc.SCENES)
def test_reductions_on_every_scene_and_kind_of_max_distance(name, kind):
    got = check_reductions(name, 64, kind=kind)
    if kind in ("zero", "negative", "nan"):  # nothing is admitted: only the dead rays of the table's zero row are occluded
        live = got["clear"][:-oc.N_DEAD]
        assert (live >= 63).all() and (live == 64).any()
    if kind == "zero" and name != "empty":
        assert not np.array_equal(got["clear"], oc.cached_model(name, 64, kind="inf")["clear"])


# ---- 4. the kernel's walk on the host ------------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime_api.h>
#include "rt_occlusion.h"
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
void probe_occlusion(uint32_t n, uint32_t n_samples, uint32_t n_table, uint32_t pass, float bias, float max_distance, const float* point,
                     const float* normal, const float* table, const uint32_t* first, uint32_t* bits, uint32_t* clear, float* visibility,
                     float* bent_normal) {
  const RtOcclusionArgs a = {point, normal, table, first, bits, clear, visibility, bent_normal, bias, max_distance, n, n_samples, n_table, pass};
  rt_occlusion_packed(g, a);
}
const char* probe_error() { return rt_last_error(); }
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("occlusion_probe")
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


def packed(probe, p, nrm, s, tab, first=None, bias=0.0, max_d=np.inf, pass_transmissive=False):
    out = oc.new_planes(p.shape[0], s, fill=0xA5)
    probe.probe_occlusion(C.c_uint32(p.shape[0]), C.c_uint32(s), C.c_uint32(tab.shape[0]), C.c_uint32(int(pass_transmissive)), C.c_float(bias),
                          C.c_float(max_d), *[C.c_void_p(ptr(a)) for a in (p, nrm, tab, first)], *[C.c_void_p(ptr(out[name])) for name in oc.PLANES])
    return out


def pack(probe, flat, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    counts = np.zeros(4, np.uint32)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(_abi.RT_SCENE_BUDGET_DEFAULT), C.c_void_p(ptr(counts)))
    assert rc == 0, probe.probe_error()
    return [int(v) for v in counts]


def twin_equals_model(probe, flat, name, state, models):
    """models: (S, first on, bias, kind, pass) -> the model's planes for `flat`, computed once per description"""
    p, nrm = oc.points(name)
    tab, first = oc.table(), oc.first(p.shape[0])
    for s, first_on, bias, kind, pt in ((33, True, 1e-4, "inf", False), (64, True, 0.0, "fraction", True), (65, False, 1e-4, "fraction", False),
                                        (7, True, 0.0, "zero", False), (2, True, 1e-4, "nan", True)):
        key = (s, first_on, bias, kind, pt)
        max_d = oc.max_distance(kind, flat)
        if key not in models:
            models[key] = oc.model(flat, p, nrm, s, tab, first if first_on else None, bias, max_d, pt)
        got = packed(probe, p, nrm, s, tab, first if first_on else None, bias, max_d, pt)
        assert oc.same_bits(got, models[key]) == [], (name, state, key)


@pytest.mark.parametrize("name", oc.SCENES)
def test_kernel_walk_equals_the_linear_scan_bit_for_bit(probe, name):
    flat = oc.scene(name)
    nt, n_slots, n_nodes, n_thr = pack(probe, flat)
    assert nt == flat.n_triangles
    models = {}
    twin_equals_model(probe, flat, name, "packed", models)
    if not flat.n_triangles:
        return
    # split clipping: several references per triangle; "some object is hit" does not count them
    nt, n_slots, n_nodes, n_thr = pack(probe, flat, bvh={"split_depth": 3})
    if name in ("text_lowres", "test_scene"):
        assert n_slots > nt, (n_slots, nt)
    twin_equals_model(probe, flat, name, "split", models)
    # after a refit to a jittered mesh: the boxes are the refit's, the answer is the jittered description's
    pack(probe, flat)
    moved = upd.jitter(flat, 0.05)
    delta, keep = _abi.make_scene_delta(moved, _abi.scene_delta_groups(flat, moved))
    assert probe.probe_refit(C.byref(delta)) == 0, probe.probe_error()
    models = {}
    twin_equals_model(probe, moved, name, "refitted", models)
    # after a rebuild, LBVH then PLOC: other trees, other slots, the same bits
    counts = np.zeros(4, np.uint32)
    for ploc in (0, 1):
        assert probe.probe_rebuild(C.c_uint32(ploc), C.c_void_p(ptr(counts))) == 0, probe.probe_error()
        twin_equals_model(probe, moved, name, "rebuilt, ploc %d" % ploc, models)


# ---- 5. known answers -----------------------------------------------------------------------------------------------------------------
def both(probe, flat):
    """-> the two implementations as call(p, nrm, s, tab, **kw)"""
    pack(probe, flat)
    return (lambda p, nrm, s, tab, **kw: oc.model(flat, p, nrm, s, tab, **kw)), (lambda p, nrm, s, tab, **kw: packed(probe, p, nrm, s, tab, **kw))


def test_known_answers(probe):
    from hslu_i.ba_raytracing.f2501_raytracer_amd import sampling

    s = 64
    tab = sampling.hemisphere_samples(s)
    assert tab.shape == (s, 3) and tab.dtype == F32 and (tab[:, 2] > 0).all() and np.abs(np.linalg.norm(tab.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert abs(float(tab[:, 2].astype(np.float64).mean()) - 2.0 / 3.0) < 0.01  # cosine-weighted: E[z] = 2/3
    # the empty scene: all clear, and the bent normal is the normal within the fixed-point step
    p, nrm = oc.points("empty")
    live = slice(0, p.shape[0] - oc.N_DEAD)
    for call in both(probe, oc.scene("empty")):
        r = call(p, nrm, s, tab, bias=1e-4)
        assert (r["clear"][live] == s).all() and (r["visibility"][live] == 1.0).all() and (r["bits"][live] == 0).all()
        o, w, _ = oc.rays_model(p, nrm, s, tab, bias=1e-4)
        mean = oc.normalize32(w[live]).astype(np.float64).sum(axis=1)
        mean /= np.linalg.norm(mean, axis=1, keepdims=True)
        # (each of the 64 terms is off by at most half a step of 2^-20 before the sum of length ~ 2 S / 3 is normalised)
        assert np.abs(r["bent_normal"][live] - mean).max() <= 2e-6
        n64 = nrm[live].astype(np.float64) / np.linalg.norm(nrm[live].astype(np.float64), axis=1, keepdims=True)
        assert np.einsum("ij,ij->i", r["bent_normal"][live].astype(np.float64), n64).min() > 0.99  # a symmetric table: the bent normal is the normal
    # the centre of a sphere: all occluded at max_distance = inf, all clear at max_distance < r
    base = oc.scene("test_scene")
    opaque = [i for i in range(base.materials.shape[0]) if base.materials[i][8] == 0.0]
    glass = [i for i in range(base.materials.shape[0]) if base.materials[i][8] != 0.0 and abs(base.materials[i][6]) > 1e-3]
    assert opaque and glass
    z3, zu = np.zeros((0, 3), F32), np.zeros((0,), np.uint32)
    ball = FlatScene(np.array([(1, 2, 3)], F32), np.array([4.0], F32), np.array([0.5], F32), np.array([opaque[0]], np.uint32), z3, z3, z3, z3, zu,
                     base.materials, base.lights).contiguous()
    p1, n1 = np.array([(1, 2, 3)], F32), np.array([(0.3, -2.0, 0.5)], F32)
    for call in both(probe, ball):
        r = call(p1, n1, s, tab)
        assert r["clear"][0] == 0 and r["visibility"][0] == 0.0 and (r["bits"][0] == 0xFFFFFFFF).all() and (r["bent_normal"][0] == 0).all()
        r = call(p1, n1, s, tab, max_d=1.9)
        assert r["clear"][0] == s and (r["bits"][0] == 0).all()
        r = call(p1, n1, s, tab, max_d=2.1)
        assert r["clear"][0] == 0
    # a point under a triangle that covers its hemisphere (the triangle spans +-1000 at height 1e-3 above the point's tangent
    # plane, the lowest sample rises 0.088 per unit): all occluded; with the triangle's material transmissive and the flag: all clear
    assert tab[:, 2].min() > 0.08
    for mat, flag, clear in ((opaque[0], False, 0), (opaque[0], True, 0), (glass[0], False, 0), (glass[0], True, s)):
        roof = FlatScene(z3, np.zeros(0, F32), np.zeros(0, F32), zu, np.array([(-1000, -1000, 1e-3)], F32), np.array([(3000, 0, 0)], F32),
                         np.array([(0, 3000, 0)], F32), np.array([(0, 0, 1)], F32), np.array([mat], np.uint32), base.materials, base.lights).contiguous()
        for call in both(probe, roof):
            r = call(np.zeros((1, 3), F32), np.array([(0, 0, 2)], F32), s, tab, pass_transmissive=flag)
            assert r["clear"][0] == clear, (mat, flag)
            r = call(np.zeros((1, 3), F32), np.array([(0, 0, -2)], F32), s, tab, pass_transmissive=flag)  # looking away from it
            assert r["clear"][0] == s


# ---- 6. validation --------------------------------------------------------------------------------------------------------------------
def test_validation_errors_and_null_planes():
    lib = _lib.load()
    flat = oc.scene("test_scene")
    desc, keep = _abi.make_scene_desc(flat)
    p, nrm = oc.points("test_scene")
    p, nrm = p[:16].copy(), nrm[:16].copy()
    s, tab = 33, oc.table()
    out = oc.new_planes(16, s, fill=0xA5)
    untouched = {name: a.copy() for name, a in out.items()}
    rays = {name: np.full(shape, 0xA5, np.uint8) for name, shape in (("o", 16 * 12), ("w", 16 * s * 12), ("alive", 16))}
    rays_untouched = {name: a.copy() for name, a in rays.items()}
    h = oc.out_struct(out)
    good = lambda **kw: oc.batch_struct(p, nrm, s, tab, **kw)  # noqa: E731

    def refused(rc, word):
        assert rc == _abi.RT_ERR_INVALID_ARG, rc
        assert word in lib.rt_last_error().decode(), lib.rt_last_error()
        assert oc.same_bits(out, untouched) == [] and oc.same_bits(rays, rays_untouched) == []  # nothing was written

    def every_call(b, word):
        """the three calls that take a description or a scene, and the rays model"""
        refused(lib.rt_ambient_occlusion_model(C.byref(desc), C.byref(b), C.byref(h)), word)
        refused(lib.rt_occlusion_rays_model(C.byref(b), ptr(rays["o"]), ptr(rays["w"]), ptr(rays["alive"])), word)

    refused(lib.rt_ambient_occlusion_model(None, C.byref(good()), C.byref(h)), "null scene")
    refused(lib.rt_ambient_occlusion(None, C.byref(good()), C.byref(h)), "null scene")
    refused(lib.rt_ambient_occlusion_device(None, C.byref(good()), C.byref(h), None), "null scene")
    refused(lib.rt_ambient_occlusion_model(C.byref(desc), None, C.byref(h)), "null occlusion batch")
    refused(lib.rt_occlusion_rays_model(None, ptr(rays["o"]), ptr(rays["w"]), ptr(rays["alive"])), "null occlusion batch")
    refused(lib.rt_ambient_occlusion_model(C.byref(desc), C.byref(good()), None), "null output")
    bad = good()
    bad.abi_version = _abi.RT_ABI_VERSION + 1
    every_call(bad, "abi_version")
    for member in ("point", "normal", "table"):
        bad = good()
        setattr(bad, member, None)
        every_call(bad, "point / normal / table missing")
    for wrong in (0, 257, 0xFFFFFFFF):
        bad = good()
        bad.n_samples = wrong
        every_call(bad, "n_samples")
    bad = good()
    bad.n_table = 0
    every_call(bad, "n_table")
    for wrong in (np.inf, -np.inf, np.nan):
        every_call(good(bias=wrong), "bias")
    for wrong in (0x2, 0x3, 0x80000000):
        every_call(good(flags=wrong), "unknown flag bits")
    refused(lib.rt_ambient_occlusion_model(C.byref(desc), C.byref(good()), C.byref(_abi.rt_occlusion_out())), "every output plane")
    # n_points == 0 is a no-op, with or without arrays
    empty = _abi.rt_occlusion_batch(_abi.RT_ABI_VERSION, 0, None, None, s, 1, None, None, 0.0, np.inf, 0)
    assert lib.rt_ambient_occlusion_model(C.byref(desc), C.byref(empty), C.byref(h)) == 0
    assert lib.rt_occlusion_rays_model(C.byref(empty), None, None, None) == 0
    assert oc.same_bits(out, untouched) == []
    # a NULL plane is not written, the others are: one plane at a time, each between guard words
    want = oc.model(flat, p, nrm, s, tab)
    for name in want:
        guarded = {m: np.full(a.size + 8, 0x5A5A5A5A, np.uint32) for m, a in want.items()}
        views = {m: guarded[m][4:-4].view(want[m].dtype).reshape(want[m].shape) for m in want}
        assert lib.rt_ambient_occlusion_model(C.byref(desc), C.byref(good()), C.byref(oc.out_struct(views, only=(name,)))) == 0, lib.rt_last_error()
        for m in want:
            assert (guarded[m][:4] == 0x5A5A5A5A).all() and (guarded[m][-4:] == 0x5A5A5A5A).all(), (name, m)
            if m == name:
                assert np.array_equal(views[m].view(np.uint32), want[m].view(np.uint32)), name
            else:
                assert (guarded[m] == 0x5A5A5A5A).all(), (name, m)


def test_header_and_exports():
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "#define RT_ABI_VERSION 4u" in text  # additive: the version stays
    assert "#define RT_MAX_OCCLUSION_SAMPLES 256u" in text and _abi.RT_MAX_OCCLUSION_SAMPLES == 256
    for name in ("rt_ambient_occlusion", "rt_ambient_occlusion_device", "rt_ambient_occlusion_model", "rt_occlusion_rays_model"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in text, name
    assert "Not offered: per-sample weights" in text


# ---- 7. the point sets are not degenerate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("test_scene", "text_lowres"))
def test_point_sets_are_not_degenerate(name):
    """A condition on the MODEL's output at S = 64 with max_distance = 0.1 of the scene's extent, bias 1e-4, the seeded table and
    start rows.  Values found: test_scene 15.0 % of all samples occluded and 56.3 % of the live points with both occluded and
    clear samples; text_lowres 17.1 % and 59.0 %."""
    occ = oc.unpack(oc.cached_model(name, 64, kind="fraction")["bits"], 64)[:-oc.N_DEAD]
    share = float(occ.mean())
    both_kinds = float((occ.any(axis=1) & ~occ.all(axis=1)).mean())
    print(name, "occluded %.3f, points with both %.3f" % (share, both_kinds))
    assert 0.10 <= share <= 0.90 and both_kinds >= 0.05
