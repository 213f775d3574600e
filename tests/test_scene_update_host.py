"""The host model of in-place scene updates (rt_refit_packed, csrc/rt_scene_pack.cpp) checked on the CPU.  It applies an
rt_scene_delta to a packed scene with the functions of csrc/rt_refit.h -- the same functions the update kernels are made
of -- so this is the specification of rt_scene_update.  The reference for every byte is a fresh rt_pack_scene of the updated
description: equal outright where a section does not depend on the tree's topology, equal through the old slot order
where it does, and for the tree itself the invariants of test_bvh_host.py plus numpy restatements of its copies.
Compiled host-only with a probe of its own, linked as test_scene_pack_host.py links: rt_scene_pack.cpp + rt_tables.cpp +
rt_bvh.cpp.  All checks are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_update_cases as cases
from test_scene_pack_host import CSRC, DEV_FIELDS, EMPTY, HIPCC, IDX, ROOT, flat_of, mesh_with_glass, ptr
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_scene_pack.h"
static RtPackedScene g[3];
extern "C" {
int probe_pack(int k, const rt_scene_desc* d, uint64_t budget, uint64_t* sizes) {
  const int rc = rt_pack_scene(d, budget, &g[k]);
  const RtRefitPlan& p = g[k].plan;
  sizes[0] = g[k].blob.size(), sizes[1] = g[k].flag_geo.size(), sizes[2] = p.height_nodes.size(), sizes[3] = p.height_offset.size();
  sizes[4] = p.thr_src.size(), sizes[5] = p.recv_cell.size(), sizes[6] = p.tri_slot.size(), sizes[7] = p.mat_class.size();
  return rc;
}
void probe_get(int k, unsigned char* blob, float* geo, uint32_t* dev, uint32_t* misc, float* aabb) {
  if (!g[k].blob.empty()) memcpy(blob, g[k].blob.data(), g[k].blob.size());
  if (!g[k].flag_geo.empty()) memcpy(geo, g[k].flag_geo.data(), g[k].flag_geo.size() * 4);
  memcpy(dev, &g[k].dev.off_spheres, 19 * 4);
  misc[0] = g[k].n_cells, misc[1] = g[k].n_tri_cells, misc[2] = g[k].plan.receivers_disabled, misc[3] = g[k].info.n_references;
  memcpy(aabb, g[k].aabb_lo, 12), memcpy(aabb + 3, g[k].aabb_hi, 12);
}
void probe_plan(int k, uint32_t* height_nodes, uint32_t* height_offset, uint32_t* thr_src, uint32_t* recv_cell, uint32_t* tri_slot, uint8_t* mat_class) {
  const RtRefitPlan& p = g[k].plan;
  auto cp = [](void* dst, const auto& v) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
  cp(height_nodes, p.height_nodes), cp(height_offset, p.height_offset), cp(thr_src, p.thr_src), cp(recv_cell, p.recv_cell);
  cp(tri_slot, p.tri_slot), cp(mat_class, p.mat_class);
}
void probe_copy(int from, int to) { g[to] = g[from]; }
int probe_refit(int k, const rt_scene_delta* d) { return rt_refit_packed(&g[k], d); }
const char* probe_error() { return rt_last_error(); }
}
'''
F32 = np.float32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("update_probe")
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


class Packed:
    pass


def get(probe, k, flat):
    p = Packed()
    p.flat = flat
    p.blob = np.zeros(int(probe._sizes[k][0]), np.uint8)
    p.geo = np.zeros(int(probe._sizes[k][1]), np.float32)
    dev, misc, aabb = np.zeros(19, np.uint32), np.zeros(4, np.uint32), np.zeros(6, np.float32)
    probe.probe_get(k, ptr(p.blob), ptr(p.geo), ptr(dev), ptr(misc), ptr(aabb))
    p.dev = {n: int(v) for n, v in zip(DEV_FIELDS, dev)}
    p.n_cells, p.n_tri_cells, p.receivers_disabled, p.n_references = (int(v) for v in misc)
    p.aabb = aabb
    return p


def pack(probe, k, flat, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    sizes = np.zeros(8, np.uint64)
    rc = probe.probe_pack(k, C.byref(desc), C.c_uint64(_abi.RT_SCENE_BUDGET_DEFAULT), ptr(sizes))
    assert rc == 0, probe.probe_error()
    if not hasattr(probe, "_sizes"):
        probe._sizes = {}
    probe._sizes[k] = sizes
    return get(probe, k, keep)


def plan_of(probe, k):
    s = [int(v) for v in probe._sizes[k]]
    a = [np.zeros(max(n, 1), np.uint32) for n in s[2:7]] + [np.zeros(max(s[7], 1), np.uint8)]
    probe.probe_plan(k, *[ptr(x) for x in a])
    names = ("height_nodes", "height_offset", "thr_src", "recv_cell", "tri_slot", "mat_class")
    return {n: x[:c] for n, x, c in zip(names, a, s[2:8])}


def refit(probe, k, old, new, full=False, groups=None):
    """applies old -> new to packed scene k; returns the return code"""
    groups = groups or _abi.scene_delta_groups(old, new, full=full)
    d, keep = _abi.make_scene_delta(new, groups)
    return probe.probe_refit(k, C.byref(d))


def section(p, off, n_records, words, dtype=np.uint32):
    o = p.dev[off]
    return p.blob[o:o + 4 * n_records * words].view(dtype).reshape(n_records, words)


SCENES = {
    "test_scene": cases.flat_test_scene,
    "semesterbild": cases.flat_semesterbild,
    "empty": lambda: flat_of().contiguous(),
    "one_triangle": lambda: flat_of(v1=[[0.1, 0.2, 0.3]], e1=[[0.5, 0.0, 0.1]], e2=[[0.0, 0.6, 0.1]], nrm=[[0, 0, 1]], tm=[0],
                                    mats=[[0.8, 0.7, 0.6, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0]], lights=[[0.5, 0.1, 0.2, 1.0, 0.9, 0.8, 3.0]]).contiguous(),
    "mesh_with_glass": lambda: mesh_with_glass().contiguous(),
}


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request):
    return request.param, SCENES[request.param]()


@pytest.fixture(scope="module", params=sorted(set(SCENES) - {"empty"}))
def movable(request):
    return request.param, SCENES[request.param]()


# ---- 1. identity --------------------------------------------------------------------------------------------------------------
def test_restating_the_creation_arrays_changes_no_byte(probe, scene):
    """pins the pad formula, the box unions, the octant swap, the threaded copy, the X arithmetic, the receiver maps, the
    material constants and the bounds in one assertion"""
    name, flat = scene
    a = pack(probe, 0, flat)
    rc = refit(probe, 0, flat, flat, full=True)
    if name == "empty":  # (no object of any kind: nothing a delta could carry)
        assert rc == _abi.RT_ERR_INVALID_ARG and b"changes nothing" in probe.probe_error()
        return
    assert rc == 0, probe.probe_error()
    b = get(probe, 0, flat)
    assert np.array_equal(a.blob, b.blob), np.flatnonzero(a.blob != b.blob)[:8]
    assert np.array_equal(a.geo.view(np.uint32), b.geo.view(np.uint32))
    assert np.array_equal(a.aabb, b.aabb) and b.receivers_disabled == 0


# ---- 2. moved geometry ----------------------------------------------------------------------------------------------------------
def padded_boxes(f):
    """rt_build_bvh's per-triangle box, float32 term for term"""
    p = np.stack([f.tri_v1, (f.tri_v1 + f.tri_e1).astype(F32), (f.tri_v1 + f.tri_e2).astype(F32)], 1)
    lo, hi = p.min(1), p.max(1)
    ext = (hi - lo).astype(F32).max(1) if len(lo) else np.zeros(0, F32)
    mag = np.maximum(np.abs(lo), np.abs(hi)).max(1) if len(lo) else np.zeros(0, F32)
    pad = ((F32(2e-5) + (F32(1e-4) * ext).astype(F32)).astype(F32) + (F32(4.0 * 1.1920929e-7) * mag).astype(F32)).astype(F32)
    return (lo - pad[:, None]).astype(F32), (hi + pad[:, None]).astype(F32)


def children(node):
    f = node.view(np.float32)
    return [(f[0:3], f[4:7], int(node[3]), int(node[7])), (f[8:11], f[12:15], int(node[11]), int(node[15]))]


def check_tree(p, f):
    """the invariants of test_bvh_host.py on a refitted tree, tightened to equalities: acyclic and complete; a leaf box IS the
    union of its triangles' padded boxes, an inner child's box IS the union of that node's child boxes; absent children
    carry NaN boxes"""
    nn, n_slots = p.dev["n_nodes"], p.dev["n_slots"]
    nodes = section(p, "off_nodes", nn, 16)
    ids = section(p, "off_tri_id", n_slots, 1)[:, 0] & IDX
    tlo, thi = padded_boxes(f)
    seen_nodes, seen_slots = set(), set()
    stack = [(0, 1)]
    while stack:
        i, depth = stack.pop()
        assert 0 <= i < nn and i not in seen_nodes and depth <= 64
        seen_nodes.add(i)
        for lo, hi, c, cnt in children(nodes[i]):
            if c == EMPTY:
                assert cnt == 0 and np.isnan(lo).all() and np.isnan(hi).all(), "an absent child keeps its NaN box"
                continue
            if cnt:
                assert c + cnt <= n_slots and not (set(range(c, c + cnt)) & seen_slots)
                seen_slots.update(range(c, c + cnt))
                t = ids[c:c + cnt]
                assert np.array_equal(lo, tlo[t].min(0)) and np.array_equal(hi, thi[t].max(0)), "leaf box = union of padded triangle boxes"
                assert (tlo[t] >= lo).all() and (thi[t] <= hi).all()
            else:
                sub = [x for x in children(nodes[c]) if x[2] != EMPTY]
                assert np.array_equal(lo, np.min([x[0] for x in sub], 0)) and np.array_equal(hi, np.max([x[1] for x in sub], 0)), \
                    "children nested in (and tight against) their parent"
                stack.append((c, depth + 1))
    assert len(seen_nodes) == nn and len(seen_slots) == n_slots
    return nodes


def expected_octants(nodes):
    nn = len(nodes)
    out = np.zeros((8, nn, 16), np.uint32)
    ch = lambda a, k: (a[:, 8 * k:8 * k + 3], a[:, 8 * k + 4:8 * k + 7], a[:, 8 * k + 3], a[:, 8 * k + 7])  # noqa: E731
    for o in range(8):
        neg = np.array([(o >> a) & 1 for a in range(3)], bool)
        rec, key = [], []
        for k in (0, 1):
            lo, hi, c, n = ch(nodes, k)
            present = (c != EMPTY)[:, None]
            lo_o, hi_o = np.where(present & neg, hi, lo), np.where(present & neg, lo, hi)
            with np.errstate(invalid="ignore"):
                terms = np.where(neg, -hi.view(F32), lo.view(F32)).astype(F32)
                kk = np.zeros(nn, F32)
                for a in range(3):
                    kk = (kk + terms[:, a]).astype(F32)
            rec.append(np.concatenate([lo_o, c[:, None], hi_o, n[:, None]], 1))
            key.append(np.where(present[:, 0], kk, F32(0)))
        both = (nodes[:, 3] != EMPTY) & (nodes[:, 11] != EMPTY)
        with np.errstate(invalid="ignore"):
            swap = both & (key[1] < key[0])
        out[o] = np.where(swap[:, None], np.concatenate([rec[1], rec[0]], 1), np.concatenate([rec[0], rec[1]], 1))
    return out.reshape(8 * nn, 16)


def expected_threaded(nodes):
    """pack_threaded_nodes restated: depth first, skip links"""
    out = []

    def node(i):
        for k in (0, 1):
            c, n = int(nodes[i, 8 * k + 3]), int(nodes[i, 8 * k + 7])
            if c == EMPTY:
                continue
            idx = len(out)
            out.append(list(nodes[i, 8 * k:8 * k + 3]) + [0] + list(nodes[i, 8 * k + 4:8 * k + 7]) + [((n << 24) | c) if n else 0])
            if not n:
                node(c)
            out[idx][3] = len(out)

    if len(nodes):
        node(0)
    return np.array(out, np.uint32).reshape(-1, 8)


def expected_bounds(f):
    r = np.sqrt(np.abs(f.sphere_r_sq))[:, None]
    pts = np.concatenate([f.sphere_center - r, f.sphere_center + r, f.tri_v1, f.tri_v1 + f.tri_e1, f.tri_v1 + f.tri_e2]).astype(F32)
    return np.concatenate([pts.min(0), pts.max(0)]) if len(pts) else np.array([0, 0, 0, 1, 1, 1], F32)


def check_against_fresh(probe, a, upd, new):
    """`upd`: the creation state `a` refitted to `new`; compared with a fresh pack of `new` (probe slot 2)"""
    fresh = pack(probe, 2, new)
    ns, nt, n_slots = new.n_spheres, new.n_triangles, a.dev["n_slots"]
    nm, nl = new.materials.shape[0], new.lights.shape[0]
    assert upd.dev == a.dev and len(upd.blob) == len(a.blob), "an update moves no section"
    # sections that do not depend on the topology: equal outright
    for off, n, words in (("off_spheres", ns, 4), ("off_sphere_rad", ns, 1), ("off_sphere_mat", ns, 1), ("off_materials", nm, 12), ("off_lights", nl, 8)):
        assert np.array_equal(section(upd, off, n, words), section(fresh, off, n, words)), off
    assert np.array_equal(section(upd, "off_tri_shade", n_slots + nt, 4)[n_slots:],
                          section(fresh, "off_tri_shade", fresh.dev["n_slots"] + nt, 4)[fresh.dev["n_slots"]:]), "canonical tri_shade"
    # slot-ordered sections: the fresh records, gathered through the OLD slot order
    ids_old = section(a, "off_tri_id", n_slots, 1)[:, 0]
    assert np.array_equal(section(upd, "off_tri_id", n_slots, 1)[:, 0], ids_old), "the slot order stays"
    t = (ids_old & IDX).astype(np.int64)
    fresh_slot_of = np.zeros(max(nt, 1), np.int64)
    fids = section(fresh, "off_tri_id", fresh.dev["n_slots"], 1)[:, 0]
    fresh_slot_of[(fids & IDX).astype(np.int64)[::-1]] = np.arange(fresh.dev["n_slots"])[::-1]
    assert np.array_equal(section(upd, "off_tri_isect", n_slots, 12), section(fresh, "off_tri_isect", fresh.dev["n_slots"], 12)[fresh_slot_of[t]])
    assert np.array_equal(section(upd, "off_tri_shade", n_slots, 4), section(fresh, "off_tri_shade", fresh.dev["n_slots"], 4)[fresh_slot_of[t]])
    assert np.array_equal(ids_old & ~np.uint32(IDX), fids[fresh_slot_of[t]] & ~np.uint32(IDX)), "flag bits as a fresh pack sets them"
    # the tree and its copies
    nodes = check_tree(upd, new)
    assert np.array_equal(section(upd, "off_nodes_oct", 8 * len(nodes), 16), expected_octants(nodes))
    assert np.array_equal(section(upd, "off_nodes_thr", upd.dev["n_thr"], 8), expected_threaded(nodes))
    assert np.array_equal(upd.aabb, expected_bounds(new)) and np.array_equal(upd.aabb, fresh.aabb)
    # receivers: the fresh maps; the R of creation or 0, never another value; the first cell of creation
    r_new, r_old, r_fresh = (section(x, "off_recv", nt, 12) for x in (upd, a, fresh))
    live = r_new[:, 8] != 0
    assert np.array_equal(r_new[live, :8], r_fresh[live, :8]), "fresh maps"
    assert (np.isin(r_new[:, 8], [0]) | (r_new[:, 8] == r_old[:, 8])).all() and np.array_equal(r_new[:, 9:], r_old[:, 9:])
    assert upd.receivers_disabled == int(((r_old[:, 8] != 0) & ~live).sum())
    # a disabled receiver is one the packer itself would not have given this R: maps not finite, or ill-conditioned
    off = (r_old[:, 8] != 0) & ~live
    assert ((r_fresh[off, 8] < r_old[off, 8]) | ~np.isfinite(r_new[off, :8].view(F32)).all(1)).all()
    if len(upd.geo):  # the flags kernel's input: new geometry, R and first cell of creation
        g_new, g_old = upd.geo.view(np.uint32).reshape(nt, 12), a.geo.view(np.uint32).reshape(nt, 12)
        u = lambda x: x.view(np.uint32).reshape(nt, 3)  # noqa: E731
        want = np.concatenate([u(new.tri_v1), g_old[:, 3:4], u(new.tri_e1), g_old[:, 7:8], u(new.tri_e2), g_old[:, 11:12]], 1)
        assert np.array_equal(g_new, want)
    return fresh


def edits(name, flat):
    rng = cases.mesh_range(name, flat)
    d = cases.diagonal(flat)
    return {"turn": cases.turn_mesh(flat, rng, 20.0, (0.02 * d, -0.01 * d, 0.015 * d)), "jitter": cases.jitter(flat, 0.05),
            "spheres_lights_material": cases.recolour(cases.orbit_lights(cases.move_spheres(flat)))}


@pytest.mark.parametrize("edit", ["turn", "jitter", "spheres_lights_material"])
def test_moved_scene_equals_a_fresh_pack_wherever_topology_does_not_matter(probe, movable, edit):
    name, flat = movable
    new = edits(name, flat)[edit]
    a = pack(probe, 0, flat)
    assert refit(probe, 0, flat, new) == 0, probe.probe_error()
    check_against_fresh(probe, a, get(probe, 0, new), new)


def test_partial_triangle_range_touches_only_its_triangles(probe):
    flat = cases.flat_semesterbild()
    first, count = flat.n_triangles // 4, flat.n_triangles // 3
    new = cases.turn_mesh(flat, (first, count), 35.0)
    assert _abi.scene_delta_groups(flat, new)["triangles"] == (first, count)
    a = pack(probe, 0, flat)
    assert refit(probe, 0, flat, new) == 0, probe.probe_error()
    check_against_fresh(probe, a, get(probe, 0, new), new)


# ---- 3. round trip ------------------------------------------------------------------------------------------------------------
def test_round_trip_restores_the_creation_blob(probe, movable):
    name, flat = movable
    a = pack(probe, 0, flat)
    moved = cases.recolour(cases.orbit_lights(cases.move_spheres(cases.jitter(flat, 0.05))))
    assert refit(probe, 0, flat, moved) == 0, probe.probe_error()
    assert not np.array_equal(get(probe, 0, moved).blob, a.blob)
    assert refit(probe, 0, moved, flat) == 0, probe.probe_error()
    b = get(probe, 0, flat)
    assert np.array_equal(a.blob, b.blob) and np.array_equal(a.geo.view(np.uint32), b.geo.view(np.uint32))
    assert np.array_equal(a.aabb, b.aabb) and b.receivers_disabled == 0


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_refit_plan_orders_children_before_parents(probe, scene):
    name, flat = scene
    a = pack(probe, 0, flat)
    pl = plan_of(probe, 0)
    nn = a.dev["n_nodes"]
    nodes = section(a, "off_nodes", nn, 16)
    assert sorted(pl["height_nodes"]) == list(range(nn)) and pl["height_offset"][0] == 0 and pl["height_offset"][-1] == nn
    height = np.zeros(nn, np.int64)
    for h in range(len(pl["height_offset"]) - 1):
        height[pl["height_nodes"][pl["height_offset"][h]:pl["height_offset"][h + 1]]] = h
    for i in range(nn):
        inner = [c for _, _, c, n in children(nodes[i]) if c != EMPTY and not n]
        assert height[i] == (1 + max(height[c] for c in inner) if inner else 0)
    assert height[0] == len(pl["height_offset"]) - 2, "the root comes last, alone"
    thr = section(a, "off_nodes_thr", a.dev["n_thr"], 8)
    src = pl["thr_src"].astype(np.int64)
    k = src & 1
    assert np.array_equal(thr[:, 0:3], np.where(k[:, None] == 0, nodes[src >> 1, 0:3], nodes[src >> 1, 8:11]))
    assert np.array_equal(thr[:, 4:7], np.where(k[:, None] == 0, nodes[src >> 1, 4:7], nodes[src >> 1, 12:15]))
    recv = section(a, "off_recv", flat.n_triangles, 12)
    assert np.array_equal(pl["recv_cell"].reshape(-1, 2), recv[:, 8:10])
    ids = section(a, "off_tri_id", a.dev["n_slots"], 1)[:, 0]
    assert np.array_equal(ids[pl["tri_slot"]] & IDX, np.arange(flat.n_triangles)) and (ids[pl["tri_slot"]] & 0x80000000 == 0).all()
    m = flat.materials
    transmissive = (m[:, 8] != 0) & ~(np.abs(m[:, 6]) <= F32(1.1920929e-7))
    used = np.isin(np.arange(len(m)), flat.tri_material)
    assert np.array_equal(pl["mat_class"], np.where(used, 2 + transmissive, 0).astype(np.uint8))


# ---- 4. validation ------------------------------------------------------------------------------------------------------------
def test_deltas_are_checked_without_a_device(probe):
    flat = mesh_with_glass().contiguous()
    pack(probe, 0, flat)
    everything = _abi.scene_delta_groups(flat, flat, full=True)
    bad = _abi.RT_ERR_INVALID_ARG

    def code(change):
        d, keep = _abi.make_scene_delta(flat, everything)
        change(d)
        return probe.probe_refit(0, C.byref(d)), probe.probe_error().decode()

    assert code(lambda d: None)[0] == 0
    assert probe.probe_refit(0, None) == bad
    rc, msg = code(lambda d: setattr(d, "abi_version", _abi.RT_ABI_VERSION + 1))
    assert rc == bad and "abi_version" in msg
    for field in _abi.SPHERE_GROUP:
        rc, msg = code(lambda d: setattr(d, field, None))
        assert rc == bad and "sphere_center" in msg and "together" in msg
    for field in _abi.TRIANGLE_GROUP:
        rc, msg = code(lambda d: setattr(d, field, None))
        assert rc == bad and "tri_v1" in msg and "together" in msg
    rc, msg = code(lambda d: setattr(d, "tri_count", 0))
    assert rc == bad and "tri_count" in msg
    rc, msg = code(lambda d: setattr(d, "tri_first", 1))
    assert rc == bad and "tri_first" in msg and "n_triangles" in msg
    rc, msg = code(lambda d: (setattr(d, "tri_first", 0xFFFFFFFF), setattr(d, "tri_count", 2)))
    assert rc == bad and "tri_first" in msg, "no 32-bit wrap-around"

    def nothing(d):
        for f in _abi.SPHERE_GROUP + _abi.TRIANGLE_GROUP + ("materials", "lights"):
            setattr(d, f, None)
        d.tri_count = 0

    rc, msg = code(nothing)
    assert rc == bad and "changes nothing" in msg
    # the transmissive class of a material in use by a triangle is fixed; of one only spheres use, free
    for row, value in ((1, 0.0), (0, 1.0), (2, 0.5)):  # glass made opaque; diffuse given an opacity; has_opacity with opacity 0 raised
        m = flat.materials.copy()
        m[row, 6] = value
        m[row, 8] = 1.0
        rc, msg = code(lambda d: setattr(d, "materials", m.ctypes.data))
        assert rc == bad and "materials" in msg and f"row {row} " in msg and "transmissive" in msg
    m = flat.materials.copy()
    m[1, 6] = 0.4  # still transmissive
    m[:, 0:3] *= 0.5
    assert code(lambda d: setattr(d, "materials", m.ctypes.data))[0] == 0
    only_spheres = flat_of(sc=[[0.3, 0.4, 0.5]], sr_sq=[0.04], sm=[0], mats=[[0.9, 0.9, 1.0, 0.0, 0.2, 1.5, 0.85, 0.1, 1.0]]).contiguous()
    pack(probe, 1, only_spheres)
    opaque = cases.copy(only_spheres, materials=np.array([[0.9, 0.9, 1.0, 0.0, 0.2, 1.5, 0.0, 0.0, 0.0]], F32))
    assert refit(probe, 1, only_spheres, opaque) == 0, probe.probe_error()


def test_split_clipped_trees_refuse_triangle_deltas_only(probe):
    flat = mesh_with_glass().contiguous()
    a = pack(probe, 0, flat, bvh=dict(split_depth=8, split_gain=0.99))
    assert a.dev["n_slots"] > flat.n_triangles
    rc = refit(probe, 0, flat, cases.jitter(flat, 0.01))
    assert rc == _abi.RT_ERR_UNSUPPORTED and b"split clipping" in probe.probe_error() and b"tri_" in probe.probe_error()
    assert np.array_equal(get(probe, 0, flat).blob, a.blob), "a refused delta changes nothing"
    new = cases.orbit_lights(cases.move_spheres(flat))
    assert refit(probe, 0, flat, new) == 0, probe.probe_error()
    upd, fresh = get(probe, 0, new), pack(probe, 2, new, bvh=dict(split_depth=8, split_gain=0.99))
    assert np.array_equal(upd.aabb, fresh.aabb)
    for off, n, words in (("off_spheres", 2, 4), ("off_sphere_rad", 2, 1), ("off_lights", 2, 8), ("off_nodes", a.dev["n_nodes"], 16)):
        assert np.array_equal(section(upd, off, n, words), section(fresh, off, n, words)), off
