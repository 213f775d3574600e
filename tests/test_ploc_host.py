"""The host model of a PLOC rebuild (rt_rebuild_ploc_packed, csrc/rt_scene_pack.cpp) checked on the CPU.  It builds the tree of
csrc/rt_ploc.h -- the functions the kernels of csrc/rt_ploc.hip are made of -- so this is the specification of
rt_scene_rebuild_with(RT_REBUILD_PLOC).  The clustering loop and everything derived from its tree (children, leaf ranges,
slots, pre-order numbers, threaded positions, depth groups, the iteration count) are held to a numpy float32 restatement
written here, with the same single-rounded operations but vectorised per iteration and with a plain depth-first walk
where the model climbs parent links; the boxes and copies are held to the refit's own checks and everything that does not
depend on the tree to the bytes it had before, as tests/test_rebuild_host.py holds the LBVH.  All checks are exact."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest

import ploc_cases as pc
import rebuild_cases as rc
import scene_update_cases as cases
from test_rebuild_host import PROBE_REBUILD, canonical_isect, check_tree_of, declare, expected_keys, info_of, padded_boxes_keep, resize, sah_of, tree_ranges
from test_scene_pack_host import CSRC, EMPTY, HIPCC, IDX, ROOT, TRANSMISSIVE, ptr
from test_scene_update_host import PROBE, children, expected_octants, expected_threaded, get, pack, plan_of, refit, section
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

F32 = np.float32
PROBE_PLOC = r'''
extern "C" int probe_rebuild_ploc(int k, uint32_t max_leaf, uint32_t radius, uint32_t* iterations) {
  return rt_rebuild_ploc_packed(&g[k], max_leaf, radius, iterations);
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("ploc_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE + PROBE_REBUILD + PROBE_PLOC)
    so = d / "probe.so"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                   [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp")],
                   check=True, capture_output=True, timeout=600)
    return declare(C.CDLL(str(so)))


# ---- driving the probe ----------------------------------------------------------------------------------------------------------
def prepared(probe, name, k=0):
    """slot k := the case as it stands before the rebuild; -> (state, plan, current flat)"""
    created, current = pc.deformed(name)
    pack(probe, k, created)
    if current is not created:
        assert refit(probe, k, created, current) == 0, probe.probe_error()
    return get(probe, k, current), plan_of(probe, k), current


def rebuilt_ploc(probe, flat, k=0, max_leaf=0, radius=0):
    """-> (state, plan, iterations)"""
    it = np.zeros(1, np.uint32)
    rc_ = probe.probe_rebuild_ploc(k, max_leaf, radius, ptr(it))
    assert rc_ == 0, probe.probe_error()
    resize(probe, k)
    return get(probe, k, flat), plan_of(probe, k), int(it[0])


# ---- the numpy restatement of csrc/rt_ploc.h ------------------------------------------------------------------------------------
def union(alo, ahi, blo, bhi):
    """box a is the cluster at the lower position: a NaN of b never replaces a's value, a NaN of a stays -> (lo, hi, distance bits)"""
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.where(blo < alo, blo, alo), np.where(ahi < bhi, bhi, ahi)
        e = (hi - lo).astype(F32)
        e = np.where(e > 0, e, F32(0))
        area = (((e[..., 0] * e[..., 1]).astype(F32) + (e[..., 1] * e[..., 2]).astype(F32)).astype(F32) + (e[..., 2] * e[..., 0]).astype(F32)).astype(F32)
    bits = np.where(np.isfinite(area), np.ascontiguousarray(area).view(np.uint32), np.uint32(0x7F800000))
    return lo, hi, bits


def expected_tree(q_sorted, radius):
    """the clustering loop over the isect records in Morton order -> (children of every inner node as {id: (a, b)}, root id,
    iterations); leaves are ids 0 .. n - 1 (the sorted positions), inner ids are this function's own"""
    n = len(q_sorted)
    lo, hi = padded_boxes_keep(types.SimpleNamespace(tri_v1=q_sorted[:, 0:3], tri_e1=q_sorted[:, 3:6], tri_e2=q_sorted[:, 6:9]))
    lo, hi = lo.astype(F32), hi.astype(F32)
    ids = np.arange(n, dtype=np.int64)
    kids, next_id, iterations = {}, n, 0
    while len(ids) > 1:
        m = len(ids)
        pos = np.arange(m, dtype=np.int64)
        key = np.full((m, 2 * radius), np.uint64(0xFFFFFFFFFFFFFFFF))
        cand = np.zeros((m, 2 * radius), np.int64)
        for k in range(1, min(radius, m - 1) + 1):
            i, j = pos[:m - k], pos[k:]
            d = union(lo[i], hi[i], lo[j], hi[j])[2].astype(np.uint64)
            pair = (d << np.uint64(32)) | (i ^ j).astype(np.uint64)
            key[i, 2 * k - 2], cand[i, 2 * k - 2] = pair, j  # (i looks up)
            key[j, 2 * k - 1], cand[j, 2 * k - 1] = pair, i  # (j looks down at the same bits)
        nn = cand[pos, key.argmin(1)]  # (all keys of a row differ: the xor does)
        mutual = nn[nn] == pos
        lower, dead = mutual & (nn > pos), mutual & (nn < pos)
        assert lower.any(), "the closest pair of all is mutual"
        a, b = pos[lower], nn[lower]
        ulo, uhi, _ = union(lo[a], hi[a], lo[b], hi[b])
        new_ids = next_id + np.arange(len(a))
        for x, ca, cb in zip(new_ids, ids[a], ids[b]):
            kids[int(x)] = (int(ca), int(cb))
        next_id += len(a)
        ids = ids.copy()
        ids[a], lo[a], hi[a] = new_ids, ulo, uhi
        keep = ~dead
        ids, lo, hi = ids[keep], lo[keep], hi[keep]
        iterations += 1
    return kids, int(ids[0]), iterations


def expected_layout(kids, root, n, max_leaf):
    """a depth-first walk, child 0 first: the sorted positions in slot order; per kept node in pre-order its (c0, n0, c1, n1) and
    depth; thr_src in threaded order"""
    size = {}
    stack = [(root, False)]  # (sizes in post-order, iteratively)
    while stack:
        x, done = stack.pop()
        if x < n:
            size[x] = 1
        elif done:
            size[x] = size[kids[x][0]] + size[kids[x][1]]
        else:
            stack += [(x, True), (kids[x][1], False), (kids[x][0], False)]
    slots, nodes, depth, thr_src = [], [], [], []
    number = {}

    def leaves_of(x):
        out, st = [], [x]
        while st:
            y = st.pop()
            if y < n:
                out.append(y)
            else:
                st += [kids[y][1], kids[y][0]]
        return out

    # pre-order with an explicit stack: ("node", x, depth) opens a kept node, ("child", r, k, depth) emits its k-th entry
    stack = [("node", root, 1)]
    while stack:
        item = stack.pop()
        if item[0] == "node":
            _, x, d = item
            r = number[x] = len(nodes)
            nodes.append([0, 0, 0, 0]), depth.append(d)
            stack += [("child", x, 1, d), ("child", x, 0, d)]
        else:
            _, x, k, d = item
            c = kids[x][k]
            thr_src.append(2 * number[x] + k)
            if size[c] <= max_leaf:
                nodes[number[x]][2 * k:2 * k + 2] = [len(slots), size[c]]
                slots += leaves_of(c)
            else:
                nodes[number[x]][2 * k:2 * k + 2] = [len(nodes), 0]
                stack.append(("node", c, d + 1))
    return np.array(slots, np.int64), np.array(nodes, np.int64), np.array(depth, np.int64), np.array(thr_src, np.int64)


def check_against_restatement(before, plan_before, after, plan_after, iterations, max_leaf, radius):
    n = before.dev["n_triangles"]
    q = canonical_isect(before, plan_before)
    keys = expected_keys(q)
    order = np.lexsort((np.arange(n), keys))
    ids = section(after, "off_tri_id", n, 1)[:, 0]
    t = (ids & IDX).astype(np.int64)
    nodes = section(after, "off_nodes", after.dev["n_nodes"], 16)
    if n <= max_leaf:
        assert np.array_equal(t, order) and iterations == 0 and after.dev["n_nodes"] == 1 and after.dev["n_thr"] == 1
        assert [(c, cnt) for _, _, c, cnt in children(nodes[0])] == [(0, n), (EMPTY, 0)], "rt_build_bvh's single root"
        return
    kids, root, want_iterations = expected_tree(q[order], radius)
    slots, want_nodes, depth, thr_src = expected_layout(kids, root, n, max_leaf)
    assert iterations == want_iterations, (iterations, want_iterations)
    assert np.array_equal(t, order[slots]), "leaf slots in depth-first order"
    assert np.array_equal(plan_after["tri_slot"][t], np.arange(n))
    assert after.dev["n_nodes"] == len(want_nodes) and after.dev["n_thr"] == 2 * len(want_nodes)
    assert np.array_equal(nodes[:, [3, 7, 11, 15]].astype(np.int64), want_nodes), "children and leaf ranges per kept node, in pre-order"
    assert np.array_equal(plan_after["thr_src"].astype(np.int64), thr_src), "threaded positions"
    want_offset = np.concatenate([[0], np.cumsum(np.bincount(depth)[:0:-1])])
    assert np.array_equal(plan_after["height_offset"].astype(np.int64), want_offset), "groups by descending depth"
    grp = plan_after["height_nodes"].astype(np.int64)
    for g in range(len(want_offset) - 1):
        part = grp[want_offset[g]:want_offset[g + 1]]
        assert np.array_equal(part, np.flatnonzero(depth == depth.max() - g)), f"group {g}: the nodes of its depth, ascending"


def check_structure(probe, before, plan_before, after, plan_after, flat, max_leaf=rc.MAX_LEAF, k=0):
    """the checks of test_rebuild_host.check_rebuilt that do not assume Morton ranges"""
    n = flat.n_triangles
    d = after.dev
    assert d["n_triangles"] == d["n_slots"] == n and d["n_spheres"] == before.dev["n_spheres"] and d["n_lights"] == before.dev["n_lights"]
    nodes = check_tree_of(after, flat)  # acyclic, complete, nested, tight = the refit of this topology
    ids = section(after, "off_tri_id", n, 1)[:, 0]
    t = (ids & IDX).astype(np.int64)
    assert np.array_equal(np.sort(t), np.arange(n)) and np.array_equal(t[plan_after["tri_slot"]], np.arange(n)), "every triangle in exactly one slot"
    ids_before = section(before, "off_tri_id", before.dev["n_slots"], 1)[:, 0]
    old_slot = plan_before["tri_slot"].astype(np.int64)[t]
    assert np.array_equal(ids & ~np.uint32(IDX), ids_before[old_slot] & np.uint32(TRANSMISSIVE))
    kept, leaves = tree_ranges(nodes)
    assert max(b - a + 1 for a, b in leaves) <= max_leaf
    ns, nm, nl = d["n_spheres"], flat.materials.shape[0], d["n_lights"]
    for off, cnt, words in (("off_spheres", ns, 4), ("off_sphere_rad", ns, 1), ("off_sphere_mat", ns, 1), ("off_recv", n, 12),
                            ("off_srecv", ns + 1, 2), ("off_materials", nm, 12), ("off_lights", nl, 8)):
        assert np.array_equal(section(after, off, cnt, words), section(before, off, cnt, words)), off
    assert np.array_equal(section(after, "off_tri_shade", 2 * n, 4)[n:], section(before, "off_tri_shade", before.dev["n_slots"] + n, 4)[before.dev["n_slots"]:])
    assert np.array_equal(after.geo.view(np.uint32), before.geo.view(np.uint32)) and np.array_equal(after.aabb.view(np.uint32), before.aabb.view(np.uint32))
    assert (after.n_cells, after.n_tri_cells, after.receivers_disabled) == (before.n_cells, before.n_tri_cells, before.receivers_disabled)
    for part in ("recv_cell", "mat_class"):
        assert np.array_equal(plan_after[part], plan_before[part]), part
    assert np.array_equal(section(after, "off_tri_isect", n, 12), section(before, "off_tri_isect", before.dev["n_slots"], 12)[old_slot])
    assert np.array_equal(section(after, "off_tri_shade", n, 4), section(before, "off_tri_shade", before.dev["n_slots"], 4)[old_slot])
    assert np.array_equal(section(after, "off_nodes_oct", 8 * len(nodes), 16), expected_octants(nodes))
    assert np.array_equal(section(after, "off_nodes_thr", d["n_thr"], 8), expected_threaded(nodes))
    off, grp = plan_after["height_offset"].astype(np.int64), plan_after["height_nodes"].astype(np.int64)
    assert sorted(grp) == list(range(d["n_nodes"])) and off[0] == 0 and off[-1] == d["n_nodes"] and (np.diff(off) > 0).all()
    group = np.zeros(d["n_nodes"], np.int64)
    for g in range(len(off) - 1):
        group[grp[off[g]:off[g + 1]]] = g
    depth = {0: 1}
    for i in range(d["n_nodes"]):  # (pre-order: a parent before its children)
        for _, _, c, cnt in children(nodes[i]):
            if c != EMPTY and not cnt:
                assert group[c] < group[i]
                depth[c] = depth[i] + 1
    assert grp[-1] == 0 and off[-1] - off[-2] == 1
    info = info_of(probe, k)
    assert info["n_nodes"] == d["n_nodes"] and info["n_leaves"] == len(leaves) and info["max_leaf_size"] == max(b - a + 1 for a, b in leaves)
    assert info["max_depth"] == (max(depth.values()) + 1 if n > max_leaf else 1) and info["n_references"] == n
    assert info["bytes_nodes"] == 64 * d["n_nodes"] and info["bytes_bvh"] == 9 * 64 * d["n_nodes"] + 32 * d["n_thr"]
    return nodes


def run_case(probe, name, radius=0, max_leaf=0):
    before, plan_before, flat = prepared(probe, name)
    after, plan_after, iterations = rebuilt_ploc(probe, flat, max_leaf=max_leaf, radius=radius)
    applied = min(max_leaf, 64) if max_leaf else rc.MAX_LEAF
    check_against_restatement(before, plan_before, after, plan_after, iterations, applied, radius or pc.RADIUS)
    check_structure(probe, before, plan_before, after, plan_after, flat, max_leaf=applied)
    return before, after, plan_after, flat, iterations


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.ALL)
def test_ploc_pack_equals_the_restatement(probe, name, record_property):
    before, after, plan_after, flat, iterations = run_case(probe, name)
    record_property(f"ploc_iterations_{name}", iterations)
    print(f"{name}: {flat.n_triangles} triangles, {iterations} iterations, {after.dev['n_nodes']} nodes, depth {info_of(probe, 0)['max_depth']}")
    # restating the geometry changes no byte, and a second rebuild neither
    assert refit(probe, 0, flat, flat, full=True) == 0, probe.probe_error()
    again = get(probe, 0, flat)
    assert np.array_equal(again.blob, after.blob), np.flatnonzero(again.blob != after.blob)[:8]
    twice, plan_twice, iterations_twice = rebuilt_ploc(probe, flat)
    assert twice.dev == after.dev and np.array_equal(twice.blob, after.blob) and iterations_twice == iterations
    for part in plan_after:
        assert np.array_equal(plan_twice[part], plan_after[part]), part


@pytest.mark.parametrize("name,radius", pc.WINDOWS)
def test_windows_clipped_at_both_ends_and_other_radii(probe, name, radius):
    run_case(probe, name, radius=radius)


@pytest.mark.parametrize("max_leaf", [1, 4, 64])
def test_other_leaf_sizes(probe, max_leaf):
    _, after, _, flat, _ = run_case(probe, "soup_100", max_leaf=max_leaf)
    if max_leaf == 1:
        assert after.dev["n_nodes"] == flat.n_triangles - 1


@pytest.mark.parametrize("n", [9, 257, 4097])
def test_equal_triangles_halve_per_iteration(probe, n):
    """derived, not measured: all distances are equal, so nn(i) = i xor 1 wherever that position exists and every iteration
    pairs all clusters but at most one -- ceil(log2 n) iterations.  A tie broken by j or |i - j| would chain: one merge each."""
    name = {9: "copies", 257: "copies_257", 4097: "copies_4097"}[n]
    before, plan_before, flat = prepared(probe, name)
    assert flat.n_triangles == n
    _, _, iterations = rebuilt_ploc(probe, flat)
    assert iterations == math.ceil(math.log2(n))


def test_a_nan_vertex_terminates(probe):
    before, after, plan_after, flat, iterations = run_case(probe, "nan_vertex")
    assert np.isnan(flat.tri_v1[7, 0]) and 0 < iterations <= flat.n_triangles - 1


def test_refusals_leave_the_pack_untouched(probe):
    before, plan_before, flat = prepared(probe, "soup_100")
    it = np.zeros(1, np.uint32)
    assert probe.probe_rebuild_ploc(0, 0, 33, ptr(it)) == _abi.RT_ERR_INVALID_ARG and b"radius" in probe.probe_error()
    assert np.array_equal(get(probe, 0, flat).blob, before.blob)
    from test_scene_pack_host import mesh_with_glass
    clipped = mesh_with_glass().contiguous()
    a = pack(probe, 0, clipped, bvh=dict(split_depth=8, split_gain=0.99))
    assert probe.probe_rebuild_ploc(0, 0, 0, ptr(it)) == _abi.RT_ERR_UNSUPPORTED and b"split clipping" in probe.probe_error()
    assert np.array_equal(get(probe, 0, clipped).blob, a.blob)


def test_a_regular_strip_runs_into_the_iteration_cap(probe):
    """on equal triangles in a row the pad of a box grows with x, so every distance to the next cluster is larger than the one
    to the previous cluster: only the pair at the low end is mutual, a few merges per iteration.  40 triangles take 25
    iterations (rebuild_cases.strip); 1000 would take about 500 and are refused at RT_PLOC_MAX_ITERATIONS = 256"""
    flat = rc.strip(1000)
    a = pack(probe, 0, flat)
    it = np.zeros(1, np.uint32)
    assert probe.probe_rebuild_ploc(0, 0, 0, ptr(it)) == _abi.RT_ERR_UNSUPPORTED and b"256 iterations" in probe.probe_error()
    assert np.array_equal(get(probe, 0, flat).blob, a.blob) and get(probe, 0, flat).dev == a.dev


def test_the_lbvh_model_is_unchanged_by_sharing_its_code(probe):
    """rt_rebuild_packed keeps every byte: the LBVH checks of test_rebuild_host on one case through this probe"""
    from test_rebuild_host import check_rebuilt, rebuilt
    before, plan_before, flat = prepared(probe, "semesterbild")
    after, plan_after = rebuilt(probe, flat)
    check_rebuilt(probe, before, plan_before, after, plan_after, flat)


# ---- SAH: exact integer sums of the host model, tri_cost 2, max_leaf 4 ----------------------------------------------------------
def sah_three(probe, created, current):
    """-> SAH (sums, value) of the refitted tree, the LBVH and PLOC (radius 8) over the same geometry, and the PLOC iterations"""
    out = []
    for method in ("refit", "lbvh", "ploc"):
        pack(probe, 0, created)
        if current is not created:
            assert refit(probe, 0, created, current) == 0, probe.probe_error()
        it = np.zeros(1, np.uint32)
        if method == "lbvh":
            assert probe.probe_rebuild(0, 0) == 0, probe.probe_error()
        if method == "ploc":
            assert probe.probe_rebuild_ploc(0, 0, 0, ptr(it)) == 0, probe.probe_error()
        resize(probe, 0)
        sums, sah, bad = sah_of(probe, 0)
        assert bad == 0
        out.append((sums, sah))
    return out[0], out[1], out[2], int(it[0])


SAH_CASES = [("semesterbild", 0.0), ("semesterbild", 0.05), ("test_scene", 0.0), ("test_scene", 0.05), ("heightfield", 0.0), ("shuffle", 0.0)]


@pytest.mark.parametrize("name,amp", SAH_CASES)
def test_ploc_costs_less_sah_than_the_lbvh(probe, name, amp, record_property):
    created, current = pc.deformed(name)
    if amp:
        current = cases.jitter(created, amp)
    refitted, lbvh, ploc, iterations = sah_three(probe, created, current)
    record_property(f"sah_{name}_{amp}", (refitted[1], lbvh[1], ploc[1], iterations))
    print(f"{name} jitter {amp:4.2f}: refitted {refitted[1]:8.2f}  LBVH {lbvh[1]:8.2f}  PLOC {ploc[1]:8.2f}  ({iterations} iterations)  "
          f"sums refitted {refitted[0]} LBVH {lbvh[0]} PLOC {ploc[0]}")
    assert ploc[1] < lbvh[1]


def test_sah_of_the_strip_is_recorded(probe, record_property):
    """recorded, not asserted: on a one-dimensional strip the Morton splits are already the best ones and PLOC is the looser tree"""
    created, current = pc.deformed("strip")
    refitted, lbvh, ploc, iterations = sah_three(probe, created, current)
    record_property("sah_strip", (refitted[1], lbvh[1], ploc[1], iterations))
    print(f"strip: as created {refitted[1]:.2f}  LBVH {lbvh[1]:.2f}  PLOC {ploc[1]:.2f}  ({iterations} iterations)")


def test_keep_better_on_the_model_level(probe):
    """what RT_REBUILD_KEEP_BETTER compares: test_scene as created -- the candidate is not lower, so it is not taken; the shuffled
    mesh -- it is"""
    created, current = pc.deformed("test_scene")
    in_place, _, ploc, _ = sah_three(probe, created, current)
    assert not ploc[1] < in_place[1], (ploc, in_place)
    created, current = pc.deformed("shuffle")
    in_place, _, ploc, _ = sah_three(probe, created, current)
    assert ploc[1] < in_place[1], (ploc, in_place)


# ---- the descriptor, through the built library: refused before the scene is looked at -------------------------------------------
@pytest.mark.parametrize("fields,word", [((2, 0, 0, 0), "method"), ((_abi.RT_REBUILD_PLOC, 33, 0, 0), "radius"), ((_abi.RT_REBUILD_LBVH, 8, 0, 0), "radius"),
                                         ((_abi.RT_REBUILD_PLOC, 0, 2, 0), "flags"), ((_abi.RT_REBUILD_PLOC, 0, 0, 1), "reserved"), (None, "rt_rebuild_desc")])
def test_descriptor_refusals_name_the_field(fields, word):
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib
    lib = _lib.load()
    desc = _abi.rt_rebuild_desc(*fields) if fields else None
    rep = _abi.rt_rebuild_report()
    for call in (lambda: lib.rt_scene_rebuild_with(None, C.byref(desc) if desc else None, C.byref(rep)),
                 lambda: lib.rt_scene_rebuild_with_device(None, C.byref(desc) if desc else None, None, C.byref(rep))):
        assert call() == _abi.RT_ERR_INVALID_ARG
        assert word in lib.rt_last_error().decode(), lib.rt_last_error()
    good = _abi.rt_rebuild_desc(_abi.RT_REBUILD_PLOC, 32, _abi.RT_REBUILD_KEEP_BETTER, 0)
    assert lib.rt_scene_rebuild_with(None, C.byref(good), None) == _abi.RT_ERR_INVALID_ARG and "null scene" in lib.rt_last_error().decode()
