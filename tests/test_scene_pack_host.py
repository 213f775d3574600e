"""The device-free half of the host side checked on the CPU: the scene packer (csrc/rt_scene_pack.cpp: every byte the kernels
read from a scene) and the builders of a frame's parameter tables (csrc/rt_tables.cpp).  Both are plain C++ without a HIP
call, compiled here host-only with a small probe and linked with rt_bvh.cpp only -- not with rt_api.cpp, which needs a
device.  All checks are exact unless a bound is named."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, distributed, sampling, scenes
from hslu_i.ba_raytracing.f2501_raytracer_amd.scene import FlatScene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_scene_pack.h"
static RtPackedScene g;
extern "C" {
int probe_check(const rt_scene_desc* d) { return rt_check_scene_desc(d); }
// sizes: [blob bytes, flag_geo floats]
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint64_t* sizes) {
  const int rc = rt_pack_scene(d, budget, &g);
  sizes[0] = g.blob.size(), sizes[1] = g.flag_geo.size();
  return rc;
}
// dev: the 19 words of RtDevScene behind `base`; misc: n_cells, n_tri_cells; aabb: lo, hi
void probe_get(unsigned char* blob, float* geo, uint32_t* dev, uint32_t* misc, uint64_t* bytes_bvh, float* aabb, rt_bvh_info* info) {
  static_assert(sizeof(RtDevScene) == 8 + 19 * 4 + 4, "RtDevScene changed: update this probe and the test's DEV_FIELDS");
  if (!g.blob.empty()) memcpy(blob, g.blob.data(), g.blob.size());
  if (!g.flag_geo.empty()) memcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4);
  memcpy(dev, &g.dev.off_spheres, 19 * 4);
  misc[0] = g.n_cells, misc[1] = g.n_tri_cells, misc[2] = g.dev.base != nullptr;
  *bytes_bvh = g.bytes_bvh;
  memcpy(aabb, g.aabb_lo, 12), memcpy(aabb + 3, g.aabb_hi, 12);
  *info = g.info;
}
uint32_t probe_aa(const float* offsets, uint32_t n, int dedup, uint32_t* out) {  // out: [4 n]
  std::vector<uint32_t> t;
  const uint32_t U = rt_build_aa_table(offsets, n, dedup != 0, &t);
  if (t.size() != 3 * (size_t)U + n) return 0xFFFFFFFFu;
  memcpy(out, t.data(), t.size() * 4);
  return U;
}
void probe_cloud(const float* cloud, uint64_t n_floats, const float* f, float* scaled, float* ball) {  // scaled: [n_floats / 3 * 4]
  std::vector<float> s;
  rt_scale_cloud(cloud, n_floats, f, &s, ball);
  memcpy(scaled, s.data(), s.size() * 4);
}
void probe_frame(float eps, float cloud_delta, const float* lo, const float* hi, float* beam, float* morton) {
  RtDevParams P{};
  P.cloud_delta = cloud_delta;
  rt_beam_constants(eps, &P);
  const float b[6] = {P.beam_delta, P.beam_delta_e5, P.beam_eps_push, P.beam_eps_ulp, P.beam_eps_o, P.beam_eps_198};
  memcpy(beam, b, sizeof(b));
  rt_morton_frame(lo, hi, morton, morton + 3);
}
uint32_t probe_super_tiles(const uint32_t* win, uint32_t tile_size, uint32_t n_ranks, uint32_t rank, const uint32_t* cost, uint32_t n_cost,
                           uint32_t* out) {
  std::vector<uint32_t> c(cost, cost + n_cost), l;
  rt_super_tiles(win, tile_size, n_ranks, rank, cost ? &c : nullptr, &l);
  if (!l.empty()) memcpy(out, l.data(), l.size() * 4);
  return (uint32_t)l.size();
}
uint32_t probe_tile_owner(uint32_t tx, uint32_t ty, uint32_t n) { return rt_tile_owner(tx, ty, n); }
const char* probe_error() { return rt_last_error(); }
}
'''
EMPTY = 0xFFFFFFFF
DUP, TRANSMISSIVE, IDX = 0x80000000, 0x40000000, 0x3FFFFFFF
F32 = np.float32
# RtDevScene behind `base`, and the sections of the blob in layout order with the bytes of one record
DEV_FIELDS = ("off_spheres", "off_sphere_rad", "off_sphere_mat", "off_tri_isect", "off_tri_shade", "off_tri_id", "off_materials", "off_lights",
              "off_nodes", "off_nodes_oct", "off_nodes_thr", "off_recv", "off_srecv", "n_thr", "n_spheres", "n_triangles", "n_lights",
              "n_nodes", "n_slots")
LAYOUT = ("off_spheres", "off_sphere_rad", "off_sphere_mat", "off_tri_isect", "off_recv", "off_srecv", "off_tri_shade", "off_tri_id",
          "off_nodes", "off_nodes_oct", "off_nodes_thr", "off_materials", "off_lights")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("pack_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    # -ffp-contract=off as in csrc/Makefile; rt_api.cpp is NOT among the sources: the packer and the table builders stand alone
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                   [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Packed:
    pass


def pack(probe, flat, budget=_abi.RT_SCENE_BUDGET_DEFAULT, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    sizes = np.zeros(2, np.uint64)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(budget), ptr(sizes))
    assert rc == 0, probe.probe_error()
    p = Packed()
    p.flat, p.budget = keep, budget
    p.blob = np.zeros(int(sizes[0]), np.uint8)
    p.geo = np.zeros(int(sizes[1]), np.float32)
    dev, misc, bytes_bvh, aabb = np.zeros(19, np.uint32), np.zeros(3, np.uint32), C.c_uint64(0), np.zeros(6, np.float32)
    p.info = _abi.rt_bvh_info()
    probe.probe_get(ptr(p.blob), ptr(p.geo), ptr(dev), ptr(misc), C.byref(bytes_bvh), ptr(aabb), C.byref(p.info))
    p.dev = {k: int(v) for k, v in zip(DEV_FIELDS, dev)}
    p.n_cells, p.n_tri_cells, p.base_set = int(misc[0]), int(misc[1]), int(misc[2])
    p.bytes_bvh, p.aabb = bytes_bvh.value, aabb
    return p


def section(p, off, n_records, words, dtype=np.uint32):
    """n_records x words 32-bit words of the blob at offset dev[off]"""
    o = p.dev[off]
    return p.blob[o:o + 4 * n_records * words].view(dtype).reshape(n_records, words)


def record_bytes(p):
    d, f = p.dev, p.flat
    return {"off_spheres": 16 * d["n_spheres"], "off_sphere_rad": 4 * d["n_spheres"], "off_sphere_mat": 4 * d["n_spheres"],
            "off_tri_isect": 48 * d["n_slots"], "off_recv": 48 * d["n_triangles"], "off_srecv": 8 * d["n_spheres"] + 8,
            "off_tri_shade": 16 * (d["n_slots"] + d["n_triangles"]), "off_tri_id": 4 * d["n_slots"], "off_nodes": 64 * d["n_nodes"],
            "off_nodes_oct": 512 * d["n_nodes"], "off_nodes_thr": 32 * d["n_thr"], "off_materials": 48 * f.materials.shape[0],
            "off_lights": 32 * f.lights.shape[0]}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def flat_of(sc=(), sr_sq=(), sm=(), v1=(), e1=(), e2=(), nrm=(), tm=(), mats=(), lights=()):
    a3 = lambda x: np.asarray(x, np.float32).reshape(-1, 3)  # noqa: E731
    r_sq = np.asarray(sr_sq, np.float32).reshape(-1)
    with np.errstate(divide="ignore"):
        r_inv = (F32(1) / np.sqrt(np.abs(r_sq))).astype(np.float32)
    return FlatScene(a3(sc), r_sq, r_inv, np.asarray(sm, np.uint32).reshape(-1), a3(v1), a3(e1), a3(e2), a3(nrm),
                     np.asarray(tm, np.uint32).reshape(-1), np.asarray(mats, np.float32).reshape(-1, 9),
                     np.asarray(lights, np.float32).reshape(-1, 7))


MAT_DIFFUSE = [0.8, 0.7, 0.6, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0]
MAT_GLASS = [0.9, 0.9, 1.0, 0.0, 0.2, 1.5, 0.85, 0.1, 1.0]
MAT_OPAQUE_SOME = [0.5, 0.5, 0.5, 0.2, 0.1, 1.3, 0.0, 0.0, 1.0]      # has_opacity, opacity 0: not transmissive
MAT_EPS_SOME = [0.5, 0.5, 0.5, 0.2, 0.1, 1.7, 1.1920929e-7, 0.0, 1.0]  # |opacity| <= epsilon: not transmissive
LIGHT = [0.5, 0.1, 0.2, 1.0, 0.9, 0.8, 3.0]


def mesh_with_glass():
    """a small soup: small triangles, some wall-sized ones across them (split candidates), slivers; a third of it transmissive"""
    r = np.random.default_rng(11)
    n = 320
    v1 = r.uniform(0, 1, (n, 3))
    s = np.where(r.random(n) < 0.15, 0.6, 0.04)[:, None]
    e1, e2 = r.normal(0, 1, (n, 3)) * s, r.normal(0, 1, (n, 3)) * s
    sl = r.random(n) < 0.1
    e2[sl] = e1[sl] * 0.7 + r.normal(0, 1e-3, (int(sl.sum()), 3))
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    tm = r.integers(0, 4, n)
    return flat_of(sc=[[0.5, 0.5, 0.5], [0.2, 0.8, 0.3]], sr_sq=[0.01, 0.0025], sm=[0, 1], v1=v1, e1=e1, e2=e2, nrm=nrm, tm=tm,
                   mats=[MAT_DIFFUSE, MAT_GLASS, MAT_OPAQUE_SOME, MAT_EPS_SOME], lights=[LIGHT, [0.1, 0.9, 0.4, 0.2, 0.3, 0.4, 1.5]])


def _scene_test():
    return scenes.test_scene(RenderConfig.from_features([])).flatten()


def _scene_semesterbild():
    return scenes.semesterbild(RenderConfig.from_features([])).flatten()


SCENES = {
    "test_scene": _scene_test,
    "semesterbild": _scene_semesterbild,
    "empty": lambda: flat_of(),
    "one_sphere": lambda: flat_of(sc=[[0.3, 0.4, 0.5]], sr_sq=[0.04], sm=[0], mats=[MAT_GLASS], lights=[LIGHT]),
    "one_triangle": lambda: flat_of(v1=[[0.1, 0.2, 0.3]], e1=[[0.5, 0.0, 0.1]], e2=[[0.0, 0.6, 0.1]], nrm=[[0, 0, 1]], tm=[0],
                                    mats=[MAT_DIFFUSE], lights=[LIGHT]),
    "zero_area_triangle": lambda: flat_of(v1=[[0.5, 0.3, 0.5], [0, 0, 0]], e1=[[0.1, 0, 0], [1, 0, 0]], e2=[[0.2, 0, 0], [0, 1, 0]],
                                          nrm=[[0, 0, 1], [0, 0, 1]], tm=[0, 1], mats=[MAT_DIFFUSE, MAT_GLASS], lights=[LIGHT]),
    "mesh_with_glass": mesh_with_glass,
}


@pytest.fixture(scope="module", params=sorted(SCENES) + ["mesh_with_glass+splits"])
def packed(request, probe):
    name, _, splits = request.param.partition("+")
    # (split clipping references a large triangle from several leaves: RT_TRI_DUPLICATE slots)
    return pack(probe, SCENES[name](), bvh=dict(split_depth=8, split_gain=0.99) if splits else None)


# ---- the scene packer --------------------------------------------------------------------------------------------------------
def test_sections_are_aligned_ordered_and_followed_by_slack(packed):
    p = packed
    size = record_bytes(p)
    assert not p.base_set, "the packer leaves RtDevScene.base null"
    assert p.dev["n_spheres"] == p.flat.n_spheres and p.dev["n_triangles"] == p.flat.n_triangles
    assert p.dev["n_lights"] == p.flat.lights.shape[0]
    for a, b in zip(LAYOUT, LAYOUT[1:] + (None,)):
        assert p.dev[a] % 256 == 0
        nxt = p.dev[b] if b else len(p.blob)
        assert nxt > p.dev[a] and nxt - (p.dev[a] + size[a]) >= 64, (a, b)
    assert p.dev[LAYOUT[0]] == 0
    assert p.bytes_bvh == 9 * 64 * p.dev["n_nodes"] + 32 * p.dev["n_thr"]
    assert (p.info.n_nodes, p.info.n_references) == (p.dev["n_nodes"], p.dev["n_slots"])
    assert p.info.bytes_nodes == 64 * p.dev["n_nodes"] and p.info.bytes_triangles == 68 * p.dev["n_slots"] + 16 * p.dev["n_triangles"]


def test_sphere_records_and_radius_bounds(packed):
    p, f = packed, packed.flat
    ns = f.n_spheres
    sp = section(p, "off_spheres", ns, 4, np.float32)
    assert np.array_equal(sp[:, :3].view(np.uint32), f.sphere_center.view(np.uint32).reshape(ns, 3))
    assert np.array_equal(sp[:, 3].view(np.uint32), f.sphere_r_sq.view(np.uint32))
    assert np.array_equal(section(p, "off_sphere_mat", ns, 1)[:, 0], f.sphere_material)
    rad = section(p, "off_sphere_rad", ns, 1, np.float32)[:, 0]
    assert (rad.astype(np.float64) >= np.sqrt(np.abs(f.sphere_r_sq.astype(np.float64)))).all()
    # bounds of everything a ray can hit
    if ns or f.n_triangles:
        r = np.sqrt(np.abs(f.sphere_r_sq))[:, None]
        pts = np.concatenate([f.sphere_center - r, f.sphere_center + r, f.tri_v1, f.tri_v1 + f.tri_e1, f.tri_v1 + f.tri_e2])
        assert np.array_equal(p.aabb[:3], pts.min(0)) and np.array_equal(p.aabb[3:], pts.max(0))
    else:
        assert np.array_equal(p.aabb, [0, 0, 0, 1, 1, 1])


def test_intersection_and_shading_records(packed):
    p, f = packed, packed.flat
    n_slots, nt = p.dev["n_slots"], f.n_triangles
    ids = section(p, "off_tri_id", n_slots, 1)[:, 0]
    t = (ids & IDX).astype(np.int64)
    assert (t < nt).all()
    isect = section(p, "off_tri_isect", n_slots, 12)
    e1, e2 = f.tri_e1[t], f.tri_e2[t]
    # X = e1 x e2 as unfused float32 a * b + (-(c * d))
    X = np.stack([e1[:, 1] * e2[:, 2] + (-(e1[:, 2] * e2[:, 1])), e1[:, 2] * e2[:, 0] + (-(e1[:, 0] * e2[:, 2])),
                  e1[:, 0] * e2[:, 1] + (-(e1[:, 1] * e2[:, 0]))], 1).astype(np.float32)
    want = np.concatenate([f.tri_v1[t], e1, e2, X], 1).astype(np.float32).reshape(n_slots, 12)
    assert np.array_equal(isect, want.view(np.uint32))
    shade = section(p, "off_tri_shade", n_slots + nt, 4)
    canon = np.concatenate([f.tri_normal.view(np.uint32).reshape(nt, 3), f.tri_material[:, None]], 1)
    assert np.array_equal(shade[n_slots:], canon), "canonical order"
    assert np.array_equal(shade[:n_slots], canon[t]), "leaf order"


def test_transmissive_bit_and_single_reference(packed):
    p, f = packed, packed.flat
    ids = section(p, "off_tri_id", p.dev["n_slots"], 1)[:, 0]
    t = (ids & IDX).astype(np.int64)
    m = f.materials[f.tri_material] if f.n_triangles else np.zeros((0, 9), np.float32)
    transmissive = (m[:, 8] != 0) & ~(np.abs(m[:, 6]) <= F32(1.1920929e-7))
    assert np.array_equal((ids & TRANSMISSIVE) != 0, transmissive[t])
    refs = np.bincount(t, minlength=f.n_triangles)
    assert (refs[transmissive] == 1).all(), "a transmissive triangle is referenced by exactly one slot"
    firsts = np.bincount(t[(ids & DUP) == 0], minlength=f.n_triangles)
    assert (firsts == 1).all(), "every triangle has exactly one first reference"


def test_split_build_references_opaque_triangles_more_than_once(probe):
    p = pack(probe, mesh_with_glass(), bvh=dict(split_depth=8, split_gain=0.99))
    ids = section(p, "off_tri_id", p.dev["n_slots"], 1)[:, 0]
    assert p.dev["n_slots"] > p.flat.n_triangles and ((ids & DUP) != 0).any(), "this scene is meant to exercise duplicate references"


def test_octant_copies_select_planes_and_put_the_near_child_first(packed):
    p = packed
    nn = p.dev["n_nodes"]
    nodes = section(p, "off_nodes", nn, 16)
    octs = section(p, "off_nodes_oct", 8 * nn, 16).reshape(8, nn, 16)
    # RtNode: lo0[3] c0 hi0[3] n0 lo1[3] c1 hi1[3] n1 -> per child: lo, hi (float bits), c, n
    child = lambda a, k: (a[..., 8 * k:8 * k + 3], a[..., 8 * k + 4:8 * k + 7], a[..., 8 * k + 3], a[..., 8 * k + 7])  # noqa: E731
    for o in range(8):
        neg = np.array([(o >> a) & 1 for a in range(3)], bool)
        exp, key = [], []
        for k in (0, 1):
            lo, hi, c, n = child(nodes, k)
            present = (c != EMPTY)[:, None]
            lo_o = np.where(present & neg, hi, lo)
            hi_o = np.where(present & neg, lo, hi)
            with np.errstate(invalid="ignore"):
                terms = np.where(neg, -hi.view(np.float32), lo.view(np.float32)).astype(np.float32)
                kk = np.zeros(nn, np.float32)
                for a in range(3):
                    kk = (kk + terms[:, a]).astype(np.float32)
            exp.append(np.concatenate([lo_o, c[:, None], hi_o, n[:, None]], 1))
            key.append(kk)
        both = (nodes[:, 3] != EMPTY) & (nodes[:, 11] != EMPTY)
        got = [np.concatenate([x[0], x[2][:, None], x[1], x[3][:, None]], 1) for x in (child(octs[o], 0), child(octs[o], 1))]
        same = (got[0] == exp[0]).all(1) & (got[1] == exp[1]).all(1)
        swapped = (got[0] == exp[1]).all(1) & (got[1] == exp[0]).all(1)
        assert (same | swapped).all(), "an octant copy holds the node's two children, planes selected"
        assert same[~both].all(), "absent children stay where and what they are"
        assert (same[both & (key[0] < key[1])]).all() and (swapped[both & (key[1] < key[0])]).all(), "smaller entry key first"


def test_threaded_copy_is_depth_first_and_covers_every_slot_once(packed):
    p = packed
    n_thr, n_slots = p.dev["n_thr"], p.dev["n_slots"]
    thr = section(p, "off_nodes_thr", n_thr, 8)
    skip, leaf = thr[:, 3].astype(np.int64), thr[:, 7]
    idx = np.arange(n_thr)
    assert (skip > idx).all() and (skip <= n_thr).all()
    assert (skip[leaf != 0] == idx[leaf != 0] + 1).all(), "a leaf is followed by its skip target"
    open_until = []  # the ends of the subtrees the walk is inside of
    for i in range(n_thr):
        while open_until and open_until[-1] == i:
            open_until.pop()
        assert not open_until or skip[i] <= open_until[-1], "subtrees nest"
        if leaf[i] == 0:
            assert skip[i] > i + 1, "an inner node has children"
            open_until.append(skip[i])
    covered = np.zeros(n_slots, np.int64)
    for lf in leaf[leaf != 0]:
        first, cnt = int(lf) & 0xFFFFFF, int(lf) >> 24
        assert first + cnt <= n_slots
        covered[first:first + cnt] += 1
    assert (covered == 1).all()


def check_receiver_grid(p):
    f, nt, ns = p.flat, p.flat.n_triangles, p.flat.n_spheres
    recv = section(p, "off_recv", nt, 12)
    R, first = recv[:, 8].astype(np.int64), recv[:, 9].astype(np.int64)
    run = np.concatenate([[0], np.cumsum(R * R)])
    assert np.array_equal(first, run[:-1] & 0xFFFFFFFF), "first cell = running sum of R * R"
    assert (R <= 1024).all() and (recv[:, 10:] == 0).all()
    assert p.n_tri_cells <= 1 << 26 and p.n_tri_cells in (0, run[-1])
    assert 2 * p.n_cells + 4 * len(p.geo) <= p.budget
    srecv = section(p, "off_srecv", ns + 1, 2)
    Rs = srecv[:ns, 0].astype(np.int64)
    assert (Rs <= 256).all() and (srecv[ns] == 0).all()
    assert np.array_equal(srecv[:ns, 1], p.n_tri_cells + np.concatenate([[0], np.cumsum(6 * Rs * Rs)])[:-1])
    assert p.n_cells == p.n_tri_cells + int((6 * Rs * Rs).sum())
    if p.n_cells:  # the input of the flags kernel: {v1, bits(R)} {e1, bits(first)} {e2, 0}
        assert p.n_tri_cells == run[-1]
        geo = p.geo.view(np.uint32).reshape(nt, 12)
        u = lambda a: a.view(np.uint32).reshape(nt, 3)  # noqa: E731
        want = np.concatenate([u(f.tri_v1), recv[:, 8:9], u(f.tri_e1), recv[:, 9:10], u(f.tri_e2), np.zeros((nt, 1), np.uint32)], 1)
        assert np.array_equal(geo, want)
    else:
        assert len(p.geo) == 0
    # the (u, v) maps, evaluated in float64: v1 -> (0, 0), v1 + e1 -> (1, 0), v1 + e2 -> (0, 1) within 0.04 / R
    big = R > 1
    m = recv[big].view(np.float32).astype(np.float64)
    v1, e1, e2 = (a[big].astype(np.float64) for a in (f.tri_v1, f.tri_e1, f.tri_e2))
    for pt, (wu, wv) in ((v1, (0, 0)), (v1 + e1, (1, 0)), (v1 + e2, (0, 1))):
        uu = (m[:, 0:3] * pt).sum(1) + m[:, 3]
        vv = (m[:, 4:7] * pt).sum(1) + m[:, 7]
        assert (np.abs(uu - wu) <= 0.04 / R[big]).all() and (np.abs(vv - wv) <= 0.04 / R[big]).all()


def test_receiver_grid(packed):
    check_receiver_grid(packed)


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("budget", [1, 40_000, 2 << 30])
def test_receiver_grid_respects_the_budget(probe, name, budget):
    p = pack(probe, SCENES[name](), budget=budget)
    check_receiver_grid(p)
    if budget == 1:
        assert p.n_cells == 0 and p.n_tri_cells == 0 and len(p.geo) == 0


def test_material_and_light_rows(packed):
    p, f = packed, packed.flat
    nm, nl = f.materials.shape[0], f.lights.shape[0]
    rows = section(p, "off_materials", nm, 12)
    assert np.array_equal(rows[:, :9], f.materials.view(np.uint32))
    ior, one = f.materials[:, 5], F32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_ior = (one / ior).astype(np.float32)
        q = ((one - ior).astype(np.float32) / (one + ior).astype(np.float32)).astype(np.float32)
        f0 = (q * q).astype(np.float32)
    assert np.array_equal(rows[:, 9], inv_ior.view(np.uint32)) and np.array_equal(rows[:, 10], f0.view(np.uint32))
    assert (rows[:, 11] == 0).all()
    li = section(p, "off_lights", nl, 8)
    want = np.concatenate([f.lights[:, 0:3], f.lights[:, 6:7], f.lights[:, 3:6], np.zeros((nl, 1), np.float32)], 1)
    assert np.array_equal(li, np.ascontiguousarray(want, np.float32).view(np.uint32))


def test_scene_description_is_checked_without_a_device(probe):
    flat = mesh_with_glass()
    null_f, null_u = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()

    def code(change):
        desc, keep = _abi.make_scene_desc(flat)
        change(desc)
        return probe.probe_check(C.byref(desc)), probe.probe_error().decode()

    assert code(lambda d: None)[0] == _abi.RT_OK
    assert probe.probe_check(None) == _abi.RT_ERR_INVALID_ARG
    bad = _abi.RT_ERR_INVALID_ARG
    assert code(lambda d: setattr(d, "abi_version", _abi.RT_ABI_VERSION + 1))[0] == bad
    for field in ("sphere_center", "sphere_r_sq", "sphere_material"):
        assert code(lambda d: setattr(d, field, null_u if field.endswith("material") else null_f)) == (bad, "sphere arrays missing")
    for field in ("tri_v1", "tri_e1", "tri_e2", "tri_normal", "tri_material"):
        assert code(lambda d: setattr(d, field, null_u if field.endswith("material") else null_f)) == (bad, "triangle arrays missing")
    assert code(lambda d: setattr(d, "materials", null_f)) == (bad, "materials missing")
    assert code(lambda d: setattr(d, "n_materials", 0)) == (bad, "materials missing")
    assert code(lambda d: setattr(d, "lights", null_f)) == (bad, "lights missing")
    assert code(lambda d: setattr(d, "sphere_r_inv", null_f))[0] == _abi.RT_OK  # (not read by the library)
    sm = flat.sphere_material.copy()
    sm[1] = 4
    assert code(lambda d: setattr(d, "sphere_material", _abi.uptr(sm))) == (bad, "sphere 1: material out of range")
    tm = flat.tri_material.copy()
    tm[17] = 4
    assert code(lambda d: setattr(d, "tri_material", _abi.uptr(tm))) == (bad, "triangle 17: material out of range")
    # a missing array of a kind the scene has none of is no error
    desc, keep = _abi.make_scene_desc(flat.without_triangles())
    desc.tri_v1 = null_f
    assert probe.probe_check(C.byref(desc)) == _abi.RT_OK


# ---- the table builders ------------------------------------------------------------------------------------------------------
CONFIG3 = ["high_resolution", "anti_aliasing", "soft_shadows"]


def aa_table(probe, offsets, dedup):
    offsets = np.ascontiguousarray(offsets, np.float32)
    n = offsets.shape[0]
    out = np.zeros(4 * n, np.uint32)
    U = probe.probe_aa(ptr(offsets), C.c_uint32(n), C.c_int(dedup), ptr(out))
    assert U != 0xFFFFFFFF, "the table is [2U | U | n] words"
    return U, out[:2 * U].view(np.float32).reshape(U, 2), out[2 * U:3 * U], out[3 * U:3 * U + n]


def test_aa_table_of_config_3_has_9_distinct_offsets(probe):
    offsets = sampling.aa_offsets(RenderConfig.from_features(CONFIG3))
    assert offsets.shape == (16, 2)
    U, uq, mult, src = aa_table(probe, offsets, True)
    assert U == 9 and int(mult.sum()) == 16 and (mult >= 1).all()
    assert (src < U).all() and (uq[src] == offsets).all(), "every sample maps to a thread with an equal offset"
    assert np.array_equal(np.bincount(src, minlength=U), mult)
    # first-occurrence order, compared as values
    first = [k for k in range(16) if not any((offsets[j] == offsets[k]).all() for j in range(k))]
    assert np.array_equal(uq.view(np.uint32), offsets[first].view(np.uint32))
    U, uq, mult, src = aa_table(probe, offsets, False)
    assert U == 16 and (mult == 1).all() and np.array_equal(src, np.arange(16))
    assert np.array_equal(uq.view(np.uint32), offsets.view(np.uint32))


def test_aa_table_compares_offsets_as_values(probe):
    U, uq, mult, src = aa_table(probe, [[0.0, 0.5], [-0.0, 0.5], [0.25, 0.5], [0.0, 0.5]], True)
    assert U == 2 and list(mult) == [3, 1] and list(src) == [0, 0, 1, 0]


def test_scaled_cloud_table_and_its_bounding_ball(probe):
    cfg = RenderConfig.from_features(CONFIG3)
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), np.float32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], np.float32)
    n = cs.size
    scaled, ball = np.zeros(n // 3 * 4, np.float32), np.zeros(4, np.float32)
    probe.probe_cloud(ptr(cs), C.c_uint64(n), ptr(f), ptr(scaled), ptr(ball))
    scaled = scaled.reshape(-1, 4)
    want = (cs.reshape(-1, 3) * f).astype(np.float32)
    assert np.array_equal(scaled[:, :3].view(np.uint32), want.view(np.uint32)), "the single float32 product"
    assert (scaled[:, 3].view(np.uint32) == 0).all()
    dist = np.linalg.norm(scaled[:, :3].astype(np.float64) - ball[:3].astype(np.float64), axis=1)
    assert ball[3] > 0 and (dist <= float(ball[3])).all()
    # (no looser than the box of the offsets needs: 0.1 % + 1e-6 above its half diagonal, up to float32 rounding)
    half = 0.5 * (want.max(0).astype(np.float64) - want.min(0).astype(np.float64))
    assert float(ball[3]) <= np.linalg.norm(half) * 1.0011 + 2e-6


def test_beam_constants_and_morton_frame(probe):
    eps, delta = F32(1e-4), F32(0.37)
    lo, hi = np.array([-1.0, 0.5, 2.0], np.float32), np.array([3.0, 0.5, 2.5], np.float32)
    beam, morton = np.zeros(6, np.float32), np.zeros(6, np.float32)
    probe.probe_frame(C.c_float(eps), C.c_float(delta), ptr(lo), ptr(hi), ptr(beam), ptr(morton))
    bd = F32(delta + F32(2.0) * eps)
    ulp = F32(F32(F32(1.3e-7) + F32(2.5e-6)) * eps)
    want = [bd, F32(bd + F32(1e-5)), F32(F32(0.998) * eps), ulp, F32(F32(F32(1.01) * eps) + F32(F32(2.0) * ulp)), F32(F32(1.98) * eps)]
    assert np.array_equal(beam.view(np.uint32), np.array(want, np.float32).view(np.uint32))
    ext = (hi - lo).astype(np.float32)
    assert np.array_equal(morton[:3], (lo - F32(0.01) * ext).astype(np.float32))
    with np.errstate(divide="ignore"):
        scale = np.where(ext > 0, F32(1024.0) / (F32(1.02) * ext).astype(np.float32), F32(0)).astype(np.float32)
    assert np.array_equal(morton[3:], scale) and morton[4] == 0, "a flat axis gets scale 0"


def super_tiles(probe, win, tile_size, n_ranks, rank, cost=None):
    win = np.asarray(win, np.uint32)
    n_all = ((int(win[2]) + 15) // 16) * ((int(win[3]) + 15) // 16)
    out = np.zeros(n_all, np.uint32)
    c = None if cost is None else np.ascontiguousarray(cost, np.uint32)
    k = probe.probe_super_tiles(ptr(win), C.c_uint32(tile_size), C.c_uint32(n_ranks), C.c_uint32(rank), None if c is None else ptr(c),
                                C.c_uint32(0 if c is None else len(c)), ptr(out))
    return out[:k].astype(np.int64), n_all


@pytest.mark.parametrize("win", [(0, 0, 100, 100), (24, 40, 100, 100)])
@pytest.mark.parametrize("tile_size", [64, 48])
@pytest.mark.parametrize("n_ranks", [1, 2, 3, 4, 5])
def test_super_tile_lists_follow_the_tile_owner(probe, win, tile_size, n_ranks):
    x0, y0, w, h = win
    st_x = (w + 15) // 16
    stride = distributed.tile_stride(n_ranks)
    owner = lambda px, py: ((px // tile_size) + stride * (py // tile_size)) % n_ranks if n_ranks > 1 else 0  # noqa: E731
    for tx, ty in ((0, 0), (1, 2), (5, 3)):
        assert probe.probe_tile_owner(tx, ty, n_ranks) == ((tx + stride * ty) % n_ranks if n_ranks > 1 else 0)
    union = set()
    for rank in range(n_ranks):
        got, n_all = super_tiles(probe, win, tile_size, n_ranks, rank)
        want = []
        for s in range(n_all):
            sx, sy = s % st_x, s // st_x
            xs = (x0 + 16 * sx, min(x0 + 16 * sx + 15, x0 + w - 1))
            ys = (y0 + 16 * sy, min(y0 + 16 * sy + 15, y0 + h - 1))
            if any(owner(px, py) == rank for px in xs for py in ys):
                want.append(s)
        assert list(got) == want, "row-major, exactly the super-tiles with a corner in one of the rank's tiles"
        union |= set(got)
    assert union == set(range(n_all))


def test_super_tiles_in_cost_order(probe):
    win = (0, 0, 100, 100)
    plain, n_all = super_tiles(probe, win, 48, 3, 1)
    cost = np.random.default_rng(3).integers(0, 5, n_all)
    got, _ = super_tiles(probe, win, 48, 3, 1, cost)
    assert list(got) == sorted(plain, key=lambda s: -cost[s]), "heaviest first, ties in row-major order"
    got, _ = super_tiles(probe, win, 48, 3, 1, cost[:-1])
    assert list(got) == list(plain), "a cost map of another window shape is not used"
