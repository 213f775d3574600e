"""The host model of a device-side BVH rebuild (rt_rebuild_packed, csrc/rt_scene_pack.cpp) checked on the CPU.  It rebuilds
the tree of a packed scene from the slot records the pack holds, with the functions of csrc/rt_lbvh.h and csrc/rt_refit.h --
the same functions the kernels are made of -- so this is the specification of rt_scene_rebuild.  The keys and the topology
are held to independent numpy restatements, the boxes and copies to the refit's own checks (test_scene_update_host.py),
everything that does not depend on the tree to the bytes it had before.  Compiled host-only with the probe of
test_scene_update_host.py plus a few functions.  All checks are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rebuild_cases as rc
import scene_update_cases as cases
from test_scene_pack_host import CSRC, EMPTY, HIPCC, IDX, ROOT, TRANSMISSIVE, mesh_with_glass, ptr
from test_scene_update_host import PROBE, check_tree, children, expected_octants, expected_threaded, get, pack, plan_of, refit, section
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

F32 = np.float32
PROBE_REBUILD = r'''
#include "rt_sah.h"
extern "C" {
int probe_rebuild(int k, uint32_t max_leaf) { return rt_rebuild_packed(&g[k], max_leaf); }
void probe_sizes(int k, uint64_t* sizes) {
  const RtRefitPlan& p = g[k].plan;
  sizes[0] = g[k].blob.size(), sizes[1] = g[k].flag_geo.size(), sizes[2] = p.height_nodes.size(), sizes[3] = p.height_offset.size();
  sizes[4] = p.thr_src.size(), sizes[5] = p.recv_cell.size(), sizes[6] = p.tri_slot.size(), sizes[7] = p.mat_class.size();
}
void probe_info(int k, uint64_t* out) {
  const rt_bvh_info& i = g[k].info;
  out[0] = i.n_nodes, out[1] = i.n_leaves, out[2] = i.max_depth, out[3] = i.max_leaf_size, out[4] = i.n_references;
  out[5] = i.bytes_nodes, out[6] = i.bytes_triangles, out[7] = g[k].bytes_bvh, out[8] = g[k].max_leaf;
}
void probe_sah(int k, uint64_t* sums, uint32_t* n_bad) { rt_sah_packed(g[k], sums, n_bad); }
}
'''
INFO = ("n_nodes", "n_leaves", "max_depth", "max_leaf_size", "n_references", "bytes_nodes", "bytes_triangles", "bytes_bvh", "max_leaf")


def declare(lib):
    lib.probe_error.restype = C.c_char_p
    lib._sizes = {}
    return lib


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("rebuild_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE + PROBE_REBUILD)
    so = d / "probe.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                   [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    return declare(C.CDLL(str(so)))


# ---- driving the probe ----------------------------------------------------------------------------------------------------------
def resize(probe, k):
    sizes = np.zeros(8, np.uint64)
    probe.probe_sizes(k, ptr(sizes))
    probe._sizes[k] = sizes


def info_of(probe, k):
    out = np.zeros(len(INFO), np.uint64)
    probe.probe_info(k, ptr(out))
    return {n: int(v) for n, v in zip(INFO, out)}


def sah_of(probe, k, tri_cost=2.0):
    sums, bad = np.zeros(2, np.uint64), np.zeros(1, np.uint32)
    probe.probe_sah(k, ptr(sums), ptr(bad))
    return (int(sums[0]), int(sums[1])), (float(sums[0]) + tri_cost * float(sums[1])) / 2.0 ** 30, int(bad[0])


def prepared(probe, name, k=0, bvh=None):
    """slot k := the case as it stands before the rebuild (created, and for "shuffle" refitted); -> (state, plan, current flat)"""
    created, current = rc.deformed(name)
    pack(probe, k, created, bvh=bvh)
    if current is not created:
        assert refit(probe, k, created, current) == 0, probe.probe_error()
    return get(probe, k, current), plan_of(probe, k), current


def rebuilt(probe, flat, k=0, max_leaf=0):
    rc_ = probe.probe_rebuild(k, max_leaf)
    assert rc_ == 0, probe.probe_error()
    resize(probe, k)
    return get(probe, k, flat), plan_of(probe, k)


# ---- the numpy restatements -----------------------------------------------------------------------------------------------------
def canonical_isect(p, plan):
    return section(p, "off_tri_isect", p.dev["n_slots"], 12, F32)[plan["tri_slot"].astype(np.int64)]


def expected_keys(q):
    """csrc/rt_lbvh.h restated in float32: centre = 0.5 (min + max) of the three vertices per axis, 10 bits per axis inside the
    bounds of the finite centres, x y z round robin from the top"""
    n = len(q)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([q[:, 0:3], (q[:, 0:3] + q[:, 3:6]).astype(F32), (q[:, 0:3] + q[:, 6:9]).astype(F32)])
        lo = np.fmin(np.fmin(np.fmin(F32(np.inf), p[0]), p[1]), p[2])
        hi = np.fmax(np.fmax(np.fmax(F32(-np.inf), p[0]), p[1]), p[2])
        c = (F32(0.5) * (lo + hi).astype(F32)).astype(F32)
    key = np.zeros(n, np.uint64)
    for a in range(3):
        fin = np.isfinite(c[:, a])
        f_lo, f_hi = (c[fin, a].min(), c[fin, a].max()) if fin.any() else (F32(np.inf), F32(-np.inf))
        if not f_hi > f_lo:
            continue  # (cell 0)
        with np.errstate(invalid="ignore", over="ignore"):
            v = (((c[:, a] - f_lo).astype(F32) / (f_hi - f_lo).astype(F32)).astype(F32) * F32(1024)).astype(F32)
        cell = np.where(v >= 1024, 1023, np.where(v >= 0, np.floor(np.where(np.isfinite(v), v, 0)), 0)).astype(np.uint64)
        cell[~fin] = 1023
        for bit in range(10):
            key |= ((cell >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - a))
    return key.astype(np.uint32)


def expected_ranges(values, max_leaf):
    """the radix tree over the sorted 62-bit values, split recursively at the highest differing bit: (kept ranges, leaf ranges)"""
    n = len(values)
    if n <= max_leaf:
        return {(0, n - 1)}, {(0, n - 1)}
    kept, leaves, stack = set(), set(), [(0, n - 1)]
    while stack:
        f, l = stack.pop()
        if l - f + 1 <= max_leaf:
            leaves.add((f, l))
            continue
        kept.add((f, l))
        bit = (values[f] ^ values[l]).bit_length() - 1
        s = f
        while (values[s + 1] >> bit) & 1 == 0:  # (values[l] has the bit set)
            s += 1
        stack += [(f, s), (s + 1, l)]
    return kept, leaves


def tree_ranges(nodes):
    """(kept ranges, leaf ranges) of a packed tree: the slots below every node"""
    kept, leaves = set(), set()

    def walk(i):
        lo, hi = 1 << 40, -1
        for _, _, c, cnt in children(nodes[i]):
            if c == EMPTY:
                continue
            a, b = (c, c + cnt - 1) if cnt else walk(c)
            if cnt:
                leaves.add((a, b))
            lo, hi = min(lo, a), max(hi, b)
        kept.add((lo, hi))
        return lo, hi

    walk(0)
    return kept, leaves


def padded_boxes_keep(f):
    """rt_grow_slot_box for geometry that is not finite: its minima and maxima never take a NaN (rt_min_keep / rt_max_keep), which
    numpy's min and max would; the same boxes as test_scene_update_host.padded_boxes wherever the geometry is finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([f.tri_v1, (f.tri_v1 + f.tri_e1).astype(F32), (f.tri_v1 + f.tri_e2).astype(F32)], 1)
        lo = np.fmin(F32(np.inf), np.fmin.reduce(p, 1))
        hi = np.fmax(F32(-np.inf), np.fmax.reduce(p, 1))
        ext = np.fmax.reduce(np.fmax(F32(0), (hi - lo).astype(F32)), 1)
        mag = np.fmax.reduce(np.fmax(F32(0), np.fmax(np.abs(lo), np.abs(hi))), 1)
        pad = ((F32(2e-5) + (F32(1e-4) * ext).astype(F32)).astype(F32) + (F32(4.0 * 1.1920929e-7) * mag).astype(F32)).astype(F32)
        return np.fmin(F32(np.inf), (lo - pad[:, None]).astype(F32)), np.fmax(F32(-np.inf), (hi + pad[:, None]).astype(F32))


def check_tree_of(p, flat):
    """check_tree; for geometry that is not finite with the NaN-free boxes of the refit"""
    if np.isfinite(flat.tri_v1).all() and np.isfinite(flat.tri_e1).all() and np.isfinite(flat.tri_e2).all():
        return check_tree(p, flat)
    import test_scene_update_host as host
    keep = host.padded_boxes
    host.padded_boxes = padded_boxes_keep
    try:
        return check_tree(p, flat)
    finally:
        host.padded_boxes = keep


def check_rebuilt(probe, before, plan_before, after, plan_after, flat, max_leaf=rc.MAX_LEAF, k=0):
    """every property a rebuilt pack has, given the pack it was made from"""
    n = flat.n_triangles
    d = after.dev
    assert d["n_triangles"] == d["n_slots"] == n and d["n_spheres"] == before.dev["n_spheres"] and d["n_lights"] == before.dev["n_lights"]
    # 1. the tree: acyclic, complete, nested, tight, NaN boxes for absent children
    nodes = check_tree_of(after, flat)
    # 2. one slot per triangle; tri_slot is the inverse of the ids
    ids = section(after, "off_tri_id", n, 1)[:, 0]
    t = (ids & IDX).astype(np.int64)
    assert np.array_equal(np.sort(t), np.arange(n)) and np.array_equal(t[plan_after["tri_slot"]], np.arange(n))
    # 3. flags: the transmissive class carried, no duplicates
    ids_before = section(before, "off_tri_id", before.dev["n_slots"], 1)[:, 0]
    old_slot = plan_before["tri_slot"].astype(np.int64)[t]
    assert np.array_equal(ids & ~np.uint32(IDX), ids_before[old_slot] & np.uint32(TRANSMISSIVE))
    # 4. no leaf larger than max_leaf
    kept, leaves = tree_ranges(nodes)
    assert max(b - a + 1 for a, b in leaves) <= max_leaf
    # 5. keys and topology against the restatements
    keys = expected_keys(canonical_isect(before, plan_before))
    order = np.lexsort((np.arange(n), keys))
    assert np.array_equal(t, order), "slots in the total order (key, canonical index)"
    values = [(int(keys[i]) << 32) | int(i) for i in order]
    want_kept, want_leaves = expected_ranges(values, max_leaf)
    assert kept == want_kept and leaves == want_leaves
    assert d["n_nodes"] == len(want_kept) and d["n_thr"] == (2 * d["n_nodes"] if n > max_leaf else 1)
    if n <= max_leaf:
        assert [(c, cnt) for _, _, c, cnt in children(nodes[0])] == [(0, n), (EMPTY, 0)], "rt_build_bvh's single root"
    # 6. canonical sections: the bytes of before
    ns, nm, nl = d["n_spheres"], flat.materials.shape[0], d["n_lights"]
    for off, cnt, words in (("off_spheres", ns, 4), ("off_sphere_rad", ns, 1), ("off_sphere_mat", ns, 1), ("off_recv", n, 12),
                            ("off_srecv", ns + 1, 2), ("off_materials", nm, 12), ("off_lights", nl, 8)):
        assert np.array_equal(section(after, off, cnt, words), section(before, off, cnt, words)), off
    assert np.array_equal(section(after, "off_tri_shade", 2 * n, 4)[n:], section(before, "off_tri_shade", before.dev["n_slots"] + n, 4)[before.dev["n_slots"]:])
    assert np.array_equal(after.geo.view(np.uint32), before.geo.view(np.uint32)) and np.array_equal(after.aabb.view(np.uint32), before.aabb.view(np.uint32))
    assert (after.n_cells, after.n_tri_cells, after.receivers_disabled) == (before.n_cells, before.n_tri_cells, before.receivers_disabled)
    for part in ("recv_cell", "mat_class"):
        assert np.array_equal(plan_after[part], plan_before[part]), part
    # 7. slot sections: the records of before, through the permutation
    assert np.array_equal(section(after, "off_tri_isect", n, 12), section(before, "off_tri_isect", before.dev["n_slots"], 12)[old_slot])
    assert np.array_equal(section(after, "off_tri_shade", n, 4), section(before, "off_tri_shade", before.dev["n_slots"], 4)[old_slot])
    # 9. the copies
    assert np.array_equal(section(after, "off_nodes_oct", 8 * len(nodes), 16), expected_octants(nodes))
    assert np.array_equal(section(after, "off_nodes_thr", d["n_thr"], 8), expected_threaded(nodes))
    # the plan: groups of children before parents, the root last and alone; thr_src mirrors the threaded copy
    off, grp = plan_after["height_offset"].astype(np.int64), plan_after["height_nodes"].astype(np.int64)
    assert sorted(grp) == list(range(d["n_nodes"])) and off[0] == 0 and off[-1] == d["n_nodes"] and (np.diff(off) > 0).all()
    group = np.zeros(d["n_nodes"], np.int64)
    for g in range(len(off) - 1):
        group[grp[off[g]:off[g + 1]]] = g
    for i in range(d["n_nodes"]):
        assert all(group[c] < group[i] for _, _, c, cnt in children(nodes[i]) if c != EMPTY and not cnt)
    assert grp[-1] == 0 and off[-1] - off[-2] == 1
    # the info: the tree's own numbers
    info = info_of(probe, k)
    depth = {0: 1}
    for i in sorted(range(d["n_nodes"]), key=lambda i: -group[i]):
        for _, _, c, cnt in children(nodes[i]):
            if c != EMPTY and not cnt:
                depth[c] = depth[i] + 1
    assert info["n_nodes"] == d["n_nodes"] and info["n_leaves"] == len(leaves) and info["max_leaf_size"] == max(b - a + 1 for a, b in leaves)
    assert info["max_depth"] == (max(depth.values()) + 1 if n > max_leaf else 1) and info["n_references"] == n
    assert info["bytes_nodes"] == 64 * d["n_nodes"] and info["bytes_bvh"] == 9 * 64 * d["n_nodes"] + 32 * d["n_thr"]
    return nodes


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.ALL)
def test_rebuilt_pack(probe, name):
    """checks 1 - 9 of the issue on every case, then 8 (an identity refit changes no byte) and 10 (a second rebuild neither)"""
    before, plan_before, flat = prepared(probe, name)
    after, plan_after = rebuilt(probe, flat)
    check_rebuilt(probe, before, plan_before, after, plan_after, flat)
    # 8. boxes, octants, threaded copy, bounds, receivers and plan are self-consistent: restating the geometry changes nothing
    assert refit(probe, 0, flat, flat, full=True) == 0, probe.probe_error()
    again = get(probe, 0, flat)
    assert np.array_equal(again.blob, after.blob), np.flatnonzero(again.blob != after.blob)[:8]
    assert np.array_equal(again.aabb.view(np.uint32), after.aabb.view(np.uint32)) and again.receivers_disabled == after.receivers_disabled
    # 10. rebuilding twice gives the same bytes
    twice, plan_twice = rebuilt(probe, flat)
    assert twice.dev == after.dev and np.array_equal(twice.blob, after.blob)
    for part in plan_after:
        assert np.array_equal(plan_twice[part], plan_after[part]), part


def test_cases_reach_the_paths_they_are_meant_for(probe):
    """no kept split, then the first one; equal keys; a centre that is not finite; two degenerate axes; three sort tiles"""
    for name, nodes in (("max_leaf", 1), ("max_leaf_plus_1", None), ("copies", None)):
        before, plan_before, flat = prepared(probe, name)
        after, _ = rebuilt(probe, flat)
        if nodes:
            assert after.dev["n_nodes"] == nodes and after.dev["n_thr"] == 1
        else:
            assert after.dev["n_nodes"] >= 1 and after.dev["n_thr"] == 2 * after.dev["n_nodes"]
    for name in ("copies", "copies_65", "copies_257", "copies_4097"):
        assert len(set(expected_keys(canonical_isect(*prepared(probe, name)[:2])))) == 1
    runs = np.bincount(np.unique(expected_keys(canonical_isect(*prepared(probe, "clusters")[:2])), return_inverse=True)[1])
    assert len(runs) == 37 and runs.min() > 64 and rc.flat_case("clusters").n_triangles == 9000 > 2 * 4096, "37 runs of equal keys, each longer than a wavefront"
    before, plan_before, flat = prepared(probe, "nan_vertex")
    keys = expected_keys(canonical_isect(before, plan_before))
    x_cell = sum(((keys >> (3 * b + 2)) & 1) << b for b in range(10))
    assert x_cell[7] == 1023 and np.isnan(flat.tri_v1[7, 0]), "the top cell"
    keys = expected_keys(canonical_isect(*prepared(probe, "strip")[:2]))
    assert (keys & np.uint32(0x1B6DB6DB)).max() == 0 and len(set(keys)) == len(keys), "y and z take cell 0"
    assert rc.flat_case("heightfield").n_triangles == 8192


def test_other_leaf_sizes(probe):
    """max_leaf 1 (every inner node kept), 2, 8 and 64 (the clamp of rt_build_bvh) on the mesh"""
    for max_leaf in (1, 2, 8, 200):
        before, plan_before, flat = prepared(probe, "semesterbild")
        after, plan_after = rebuilt(probe, flat, max_leaf=max_leaf)
        nodes = check_rebuilt(probe, before, plan_before, after, plan_after, flat, max_leaf=min(max_leaf, 64))
        if max_leaf == 1:
            assert len(nodes) == flat.n_triangles - 1


def test_transmissive_flags_are_carried(probe):
    before, plan_before, flat = prepared(probe, "mesh_with_glass")
    after, _ = rebuilt(probe, flat)
    ids = section(after, "off_tri_id", flat.n_triangles, 1)[:, 0]
    m = flat.materials[flat.tri_material[(ids & IDX).astype(np.int64)]]
    transmissive = (m[:, 8] != 0) & ~(np.abs(m[:, 6]) <= F32(1.1920929e-7))
    assert transmissive.any() and not transmissive.all()
    assert np.array_equal((ids & TRANSMISSIVE) != 0, transmissive) and (ids & 0x80000000 == 0).all()


# ---- 11. refusals and SAH ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_pack_untouched(probe):
    flat = mesh_with_glass().contiguous()
    a = pack(probe, 0, flat, bvh=dict(split_depth=8, split_gain=0.99))
    assert a.dev["n_slots"] > flat.n_triangles
    assert probe.probe_rebuild(0, 0) == _abi.RT_ERR_UNSUPPORTED and b"split clipping" in probe.probe_error()
    assert np.array_equal(get(probe, 0, flat).blob, a.blob) and get(probe, 0, flat).dev == a.dev
    from test_scene_pack_host import flat_of
    only_spheres = flat_of(sc=[[0.3, 0.4, 0.5]], sr_sq=[0.04], sm=[0], mats=[[0.9, 0.9, 1.0, 0.0, 0.2, 1.5, 0.85, 0.1, 1.0]]).contiguous()
    b = pack(probe, 1, only_spheres)
    assert probe.probe_rebuild(1, 0) == _abi.RT_ERR_INVALID_ARG and b"nothing to rebuild" in probe.probe_error()
    assert np.array_equal(get(probe, 1, only_spheres).blob, b.blob)
    # A tree too deep for the traversal stack cannot be constructed, below 10 000 triangles or above: the radix tree splits
    # on the 30 bits of the key and then on the bits of the canonical index, 23 at most (RT_LBVH_MAX_TRIANGLES), so a kept
    # node is at most 53 deep and max_depth + 2 <= 56.  The refusal in rt_rebuild_shape is a guard; the deepest tree of the
    # cases is printed below.
    before, plan_before, flat = prepared(probe, "copies")
    rebuilt(probe, flat, max_leaf=1)
    print("deepest tree of 9 equal triangles, max_leaf 1:", info_of(probe, 0)["max_depth"])
    assert info_of(probe, 0)["max_depth"] == 5, "9 indices: 4 bits, and the leaves below"


def test_rebuild_repairs_a_shuffled_tree(probe):
    """the same triangle soup in a tree that groups strangers: the rebuilt tree costs less than the refitted one.  An
    ordering, not a tolerance"""
    before, _, flat = prepared(probe, "shuffle")
    q_refit, sah_refit, bad = sah_of(probe, 0)
    rebuilt(probe, flat)
    q_rebuilt, sah_rebuilt, bad2 = sah_of(probe, 0)
    pack(probe, 2, flat)
    _, sah_fresh, _ = sah_of(probe, 2)
    print(f"shuffle: SAH refitted {sah_refit:.2f}, rebuilt {sah_rebuilt:.2f}, fresh {sah_fresh:.2f}")
    assert bad == bad2 == 0 and sah_rebuilt < sah_refit


@pytest.mark.parametrize("name", ["semesterbild", "test_scene"])
def test_sah_along_the_jitter_amplitudes_is_recorded(probe, name, record_property):
    """recorded, not asserted: SAH of the refitted, the rebuilt and a fresh tree per jitter amplitude (profiles/rebuild.md)"""
    flat = rc.flat_case(name)
    for amp in (0.0, 0.01, 0.02, 0.05, 0.1):
        new = cases.jitter(flat, amp) if amp else flat
        pack(probe, 0, flat)
        if amp:
            assert refit(probe, 0, flat, new) == 0, probe.probe_error()
        _, refitted, _ = sah_of(probe, 0)
        rebuilt(probe, new)
        _, again, _ = sah_of(probe, 0)
        pack(probe, 2, new)
        _, fresh, _ = sah_of(probe, 2)
        record_property(f"sah_{name}_{amp}", (refitted, again, fresh))
        print(f"{name} jitter {amp:4.2f}: refitted {refitted:8.2f}  rebuilt {again:8.2f}  fresh {fresh:8.2f}  rebuilt/refitted {again / refitted:.3f}")
