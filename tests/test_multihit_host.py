"""Multi-hit ray queries on the CPU.  rt_list_intersections_model (the specification: a linear scan with csrc/rt_multihit.h)
bit for bit against tests/multi_hit_ref.c -- the oracle's own intersection tests, a sort and the cursor; rt_multihit_packed (the
KERNEL's walk -- spheres, threaded walk with the slab test, passes for `total` -- run on the host over the packed blob) bit for
bit against the model on blobs packed plain, split-clipped and rebuilt, which is what shows that the pruning never cuts a hit
or a tie; answers known by hand; paging through the cursor; and the validation errors.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import multi_hit_cases as mh
import ray_query_cases as rq
import scene_update_cases as upd
from test_scene_pack_host import CSRC, HIPCC, ROOT
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

F32 = np.float32
ptr = mh.ptr


# ---- 1. the model against the oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nearest_ref(tmp_path_factory):
    return rq.build_ref(tmp_path_factory.mktemp("ray_query_ref"))


@pytest.mark.parametrize("cull", (False, True))
@pytest.mark.parametrize("name", mh.SCENES)
def test_model_equals_the_oracle_bit_for_bit(nearest_ref, name, cull):
    flat = mh.scene(name)
    o, d = mh.rays(name)
    free = mh.ref(flat, o, d, 16, cull=cull)
    second = free["t"][:, 1].copy()
    small = name == "text"  # (14569 triangles: a linear scan of 1021 rays takes seconds, so fewer combinations)
    for k in (2, 16) if small else mh.KS:  # every K, with total
        assert mh.same_bits(mh.model(flat, o, d, k, cull=cull), mh.ref(flat, o, d, k, cull=cull)) == [], k
    for kind in ("mixed",) if small else mh.MAX_D:  # every kind of max_distance, with and without total
        m = mh.max_distance(kind, flat, o, second)
        for k, total in ((5, True),) if small else ((5, True), (2, False)):
            got, want = mh.model(flat, o, d, k, m, cull, total=total), mh.ref(flat, o, d, k, m, cull, total=total)
            assert mh.same_bits(got, want) == [], (kind, k, total)
            if kind in ("negative", "nan"):
                assert (got["count"] == 0).all() and (got["id"] == -1).all()
            if kind in ("none", "inf") and total:
                assert np.array_equal(got["total"], free["total"])
    if not small:
        assert mh.same_bits(mh.model(flat, o, d, 16, cull=cull, total=False), mh.ref(flat, o, d, 16, cull=cull, total=False)) == []
    # entry 0 with K = 1 is the nearest hit of the ray queries' reference
    one = mh.model(flat, o, d, 1, cull=cull)
    near = rq.ref_nearest(nearest_ref, flat, o, d, cull=cull)
    for plane in ("id", "t", "point", "normal", "material"):
        assert np.array_equal(one[plane].reshape(near[plane].shape).view(np.uint32), near[plane].view(np.uint32)), plane
    # the properties of every list: count = min(total, K), miss values behind it, dead rays empty, keys in order
    got = mh.model(flat, o, d, 5, cull=cull)
    assert np.array_equal(got["count"], np.minimum(got["total"], 5))
    behind = np.arange(5)[None, :] >= got["count"][:, None]
    assert (got["id"][behind] == -1).all() and (got["t"][behind] == np.inf).all() and (got["material"][behind] == 0xFFFFFFFF).all()
    assert (got["point"][behind].view(np.uint32) == 0).all() and (got["normal"][behind].view(np.uint32) == 0).all()
    assert (got["count"][-4:] == 0).all() and (got["total"][-4:] == 0).all()
    t, i = got["t"].astype(np.float64), got["id"].astype(np.int64)
    both = ~behind[:, 1:]
    assert ((t[:, :-1] < t[:, 1:]) | ((t[:, :-1] == t[:, 1:]) & (i[:, :-1] > i[:, 1:])))[both].all()
    if name in ("test_scene", "text_lowres") and not cull:  # the ray set is not degenerate
        share2, share5 = float((free["total"] >= 2).mean()), float((free["total"] > 4).mean())
        print(name, "rays with >= 2 hits %.3f, with > 4 hits %.3f, most hits %d" % (share2, share5, int(free["total"].max())))
        assert share2 >= 0.40 and share5 >= 0.05


# ---- 2. the kernel's walk on the host -------------------------------------------------------------------------------------------
PROBE = r'''
#include <hip/hip_runtime_api.h>
#include "rt_multihit.h"
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
void probe_multihit(uint32_t n, uint32_t max_hits, uint32_t cull, const float* origin, const float* direction, const float* max_distance,
                    const float* after_t, const int32_t* after_id, uint32_t* count, uint32_t* total, int32_t* id, float* t, float* point,
                    float* normal, uint32_t* material) {
  const RtMultiHitArgs a = {origin, direction, max_distance, after_t, after_id, count, total, id, t, point, normal, material, n, max_hits, cull};
  rt_multihit_packed(g, a);
}
const char* probe_error() { return rt_last_error(); }
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("multihit_probe")
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


def packed(probe, o, d, k, max_d=None, cull=False, after=None, total=True):
    out = mh.new_planes(o.shape[0], k)
    at, ai = after if after is not None else (None, None)
    probe.probe_multihit(C.c_uint32(o.shape[0]), C.c_uint32(k), C.c_uint32(int(cull)), *[C.c_void_p(ptr(a)) for a in (o, d, max_d, at, ai)],
                         C.c_void_p(ptr(out["count"])), C.c_void_p(ptr(out["total"]) if total else None),
                         *[C.c_void_p(ptr(out[name])) for name, _, _ in mh.LIST_PLANES])
    if not total:
        out["total"] = None
    return out


def pack(probe, flat, bvh=None):
    desc, keep = _abi.make_scene_desc(flat, bvh=bvh)
    counts = np.zeros(4, np.uint32)
    rc = probe.probe_pack(C.byref(desc), C.c_uint64(_abi.RT_SCENE_BUDGET_DEFAULT), C.c_void_p(ptr(counts)))
    assert rc == 0, probe.probe_error()
    return [int(v) for v in counts]


_MODEL = {}


def cached_model(flat, o, d, k, max_d=None, cull=False, after=None, total=True):
    """the model's planes of a call, computed once per description (two tree states of one description ask for the same lists)"""
    key = (id(flat), k, cull, total, None if max_d is None else max_d.tobytes(), None if after is None else after[0].tobytes() + after[1].tobytes())
    if key not in _MODEL:
        _MODEL[key] = (flat, mh.model(flat, o, d, k, max_d, cull, after, total))
    return _MODEL[key][1]


def twin_equals_model(probe, flat, o, d, state, small=False):
    """small (the 14569 triangles of `text`, where a linear scan takes seconds): K = 5 and 16 without culling only"""
    second = cached_model(flat, o, d, 2)["t"][:, 1].copy()
    mixed = mh.max_distance("mixed", flat, o, second)
    for cull in (False,) if small else (False, True):
        for k in (5, 16) if small else mh.KS:
            assert mh.same_bits(packed(probe, o, d, k, cull=cull), cached_model(flat, o, d, k, cull=cull)) == [], (state, cull, k)
        assert mh.same_bits(packed(probe, o, d, 5, mixed, cull), cached_model(flat, o, d, 5, mixed, cull)) == [], (state, cull, "mixed")
        assert mh.same_bits(packed(probe, o, d, 2, mixed, cull, total=False), cached_model(flat, o, d, 2, mixed, cull, total=False)) == [], (state, cull)
    # behind a cursor: the last key of each row of a K = 2 call
    first = cached_model(flat, o, d, 2)
    has = first["count"] > 0
    last = np.maximum(first["count"].astype(np.int64) - 1, 0)
    rows = np.arange(o.shape[0])
    after = (np.where(has, first["t"][rows, last], F32(np.nan)).astype(F32), np.where(has, first["id"][rows, last], 0).astype(np.int32))
    assert mh.same_bits(packed(probe, o, d, 5, after=after), cached_model(flat, o, d, 5, after=after)) == [], (state, "cursor")


@pytest.mark.parametrize("name", mh.SCENES)
def test_kernel_walk_equals_the_linear_scan_bit_for_bit(probe, name):
    """the rays of mh.rays hold the 100-extent, grazing, on-surface and zero-component kinds"""
    flat = mh.scene(name)
    o, d = mh.rays(name)
    nt, n_slots, n_nodes, n_thr = pack(probe, flat)
    assert nt == flat.n_triangles
    twin_equals_model(probe, flat, o, d, "packed", name == "text")
    if not flat.n_triangles:
        return
    if name != "text":  # (refitting and rebuilding the 14569 triangles of `text` on the host takes a minute; text_lowres is the same mesh at 1687)
        # after a refit to a jittered mesh: the boxes are the refit's, the answer is the jittered description's
        moved = upd.jitter(flat, 0.05)
        delta, keep = _abi.make_scene_delta(moved, _abi.scene_delta_groups(flat, moved))
        assert probe.probe_refit(C.byref(delta)) == 0, probe.probe_error()
        twin_equals_model(probe, moved, o, d, "refitted")
        # after a rebuild: another tree, other slots, the same bits
        counts = np.zeros(4, np.uint32)
        assert probe.probe_rebuild(C.c_void_p(ptr(counts))) == 0, probe.probe_error()
        twin_equals_model(probe, moved, o, d, "rebuilt")
    # split clipping: several references per triangle, each evaluates the whole triangle and is listed once
    nt, n_slots, n_nodes, n_thr = pack(probe, flat, bvh={"split_depth": 3})
    if name in ("text_lowres", "text", "test_scene"):
        assert n_slots > nt, (n_slots, nt)  # n_references > n_triangles
    twin_equals_model(probe, flat, o, d, "split", name == "text")
    _MODEL.clear()


# ---- 3. known answers -------------------------------------------------------------------------------------------------------------
def layer_ray(n=1):
    return np.tile(F32(mh.LAYER_ORIGIN), (n, 1)), np.tile(F32(mh.LAYER_DIR), (n, 1))


def test_known_answers_of_the_layered_scene(probe):
    flat = mh.scene("layers")
    ids, ts = mh.layers_answer()
    assert len(ids) == 42 and ids[10:12] == [12, 11] and ts[10:12] == [10.0, 10.0]  # the coincident pair: larger id first
    o, d = layer_ray()
    pack(probe, flat)
    for call in (lambda **kw: mh.model(flat, o, d, 16, **kw), lambda **kw: packed(probe, o, d, 16, **kw)):
        r = call()
        assert r["count"][0] == 16 and r["total"][0] == 42
        assert r["id"][0].tolist() == ids[:16] and r["t"][0].tolist() == ts[:16]
        assert np.array_equal(r["point"][0], np.array([[0.25, 0.25, t] for t in ts[:16]], F32))
        assert np.array_equal(r["normal"][0], np.tile(F32([0, 0, 1]), (16, 1)))  # (the ray leaves sphere 0 through its pole)
        assert r["material"][0, 0] == flat.sphere_material[0] and r["material"][0, 1] == flat.tri_material[0]
        # K = 16 paging through `after`: the whole sequence, no gap, no repeat
        keys, _ = mh.chain(lambda after: call(after=after), 1, 16)
        assert [k[1] for k in keys[0]] == ids and np.array(([k[0] for k in keys[0]]), np.uint32).view(F32).tolist() == ts
        # a cursor AT the first of the coincident pair resumes with the second
        r = call(after=(F32([10.0]), np.int32([12])))
        assert r["id"][0, :3].tolist() == [11, 13, 14] and r["total"][0] == 42 - 11
        r = call(after=(F32([10.0]), np.int32([11])))
        assert r["id"][0, :2].tolist() == [13, 14] and r["total"][0] == 42 - 12
        # max_distance is inclusive; the cursor (NaN, anything) admits nothing
        r = call(max_d=F32([10.0]))
        assert r["total"][0] == 12 and r["id"][0, :12].tolist() == ids[:12] and (r["id"][0, 12:] == -1).all()
        r = call(after=(F32([np.nan]), np.int32([5])))
        assert r["count"][0] == 0 and r["total"][0] == 0
    # culling: the ray hits every triangle head-on from behind (dot(d, n) = 1 >= 0.75) and leaves sphere 0 from inside (dot = 1):
    # only the front of sphere 1 (dot = -1) counts, every material here being opaque
    r = mh.model(flat, o, d, 16, cull=True)
    assert r["total"][0] == 1 and r["id"][0, 0] == 1 and r["t"][0, 0] == F32(48.0)


# ---- 4. paging ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 4))
def test_paging_reproduces_the_full_sorted_list(k):
    flat = mh.scene("test_scene")
    o, d = mh.rays("test_scene")
    n = o.shape[0]
    full = mh.ref(flat, o, d, 16)  # no ray of this set has more than 16 hits on test_scene
    assert int(full["total"].max()) <= 16
    keys, first = mh.chain(lambda after: mh.model(flat, o, d, k, after=after), n, k)
    assert np.array_equal(first["total"], full["total"])
    for i in range(n):
        c = int(full["total"][i])
        assert keys[i] == list(zip(full["t"][i, :c].view(np.uint32).tolist(), full["id"][i, :c].tolist())), i


# ---- 5. validation --------------------------------------------------------------------------------------------------------------------
def test_validation_errors_and_null_planes():
    lib = _lib.load()
    flat = mh.scene("test_scene")
    desc, keep = _abi.make_scene_desc(flat)
    o, d = mh.rays("test_scene")
    o, d = o[:16].copy(), d[:16].copy()
    k = 4
    out = mh.new_planes(16, k, fill=0xA5)
    untouched = {name: a.copy() for name, a in out.items()}
    b, h = mh.batch_struct(o, d), mh.lists_struct(out, k)

    def refused(rc, word):
        assert rc == _abi.RT_ERR_INVALID_ARG, rc
        assert word in lib.rt_last_error().decode(), lib.rt_last_error()
        assert mh.same_bits(out, untouched) == []  # nothing was written

    refused(lib.rt_list_intersections_model(None, C.byref(b), C.byref(h)), "null scene")
    refused(lib.rt_list_intersections(None, C.byref(b), C.byref(h)), "null scene")
    refused(lib.rt_list_intersections_device(None, C.byref(b), C.byref(h), None), "null scene")
    refused(lib.rt_list_intersections_model(C.byref(desc), None, C.byref(h)), "null ray batch")
    refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(b), None), "null output")
    bad = mh.batch_struct(o, d)
    bad.abi_version = _abi.RT_ABI_VERSION + 1
    refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(bad), C.byref(h)), "abi_version")
    bad = mh.batch_struct(o, d)
    bad.direction = None
    refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(bad), C.byref(h)), "origin / direction missing")
    bad = mh.batch_struct(o, d)
    bad.flags = _abi.RT_FLAG_BACKFACE_CULLING | 0x1
    refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(bad), C.byref(h)), "unknown flag bits")
    for wrong in (0, 17, 0xFFFFFFFF):
        refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(b), C.byref(mh.lists_struct(out, wrong))), "max_hits")
    cur_t, cur_id = np.zeros(16, F32), np.zeros(16, np.int32)
    for after in ((cur_t, None), (None, cur_id)):
        refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(b), C.byref(mh.lists_struct(out, k, after=after))), "after_t and after_id")
    none = _abi.rt_ray_hit_lists()
    none.max_hits = k
    refused(lib.rt_list_intersections_model(C.byref(desc), C.byref(b), C.byref(none)), "every output plane")
    # n_rays == 0 is a no-op, with or without arrays
    empty = _abi.rt_ray_batch()
    empty.abi_version = _abi.RT_ABI_VERSION
    assert lib.rt_list_intersections_model(C.byref(desc), C.byref(empty), C.byref(h)) == 0
    assert mh.same_bits(out, untouched) == []
    # a NULL plane is not written, the others are: one plane at a time, each between guard words
    want = mh.model(flat, o, d, k)
    for name in want:
        guarded = {m: np.full(a.size + 8, 0x5A5A5A5A, np.uint32) for m, a in want.items()}
        views = {m: guarded[m][4:-4].view(want[m].dtype).reshape(want[m].shape) for m in want}
        one = mh.lists_struct(views, k, only=(name,))
        assert lib.rt_list_intersections_model(C.byref(desc), C.byref(b), C.byref(one)) == 0, lib.rt_last_error()
        for m in want:
            assert (guarded[m][:4] == 0x5A5A5A5A).all() and (guarded[m][-4:] == 0x5A5A5A5A).all(), (name, m)
            if m == name:
                assert np.array_equal(views[m].view(np.uint32), want[m].view(np.uint32)), name
            else:
                assert (guarded[m] == 0x5A5A5A5A).all(), (name, m)
