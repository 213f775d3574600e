"""The device half of "one arithmetic, compiled twice" (csrc/rt_refit.h), measured: the kernels of csrc/rt_update.hip held
byte for byte to rt_refit_packed, the host model that tests/test_scene_update_host.py holds to a fresh rt_pack_scene.
A probe links against the built librt_hip.so -- it takes rt_pack_scene, rt_refit_packed, rt_check_scene_delta and
rt_launch_update from the library, so the kernels driven here are the ones that ship -- uploads a packed scene, applies a
delta with rt_launch_update and reads everything back: every word of the blob, every word of flag_geo, the six bounds and
the counter of disabled receivers.  All comparisons are array_equal on 32-bit words.  One exemption, only where a test
asks for it and only inside float words: two words that are both NaN as fp32 count as equal (inf - inf has another sign
bit on x86 than on the GPU); by construction the host word is a NaN wherever it is used.
The preconditions of the cases (is every class of value present? is the counter strictly between nothing and everything?)
are host-side and run without a GPU."""
import ctypes as C
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import scene_update_cases as cases
from test_scene_pack_host import CSRC, EMPTY, HIPCC, IDX, LAYOUT, LIGHT, MAT_DIFFUSE, ROOT, flat_of, record_bytes
from test_scene_update_host import (SCENES, check_against_fresh, check_tree, children, edits, expected_bounds, expected_octants, expected_threaded, get, pack, plan_of,
                                    refit, section)
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi, _lib

gpu = pytest.mark.gpu
F32 = np.float32
HIP_ERROR = 1000  # probe return codes: 0, an RT_ERR_* (negative), HIP_ERROR + hipError_t, or -100 (the probe was misused)

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_scene_pack.h"
static RtPackedScene g[8];
extern "C" {
int probe_pack(int k, const rt_scene_desc* d, uint64_t budget, uint64_t* sizes) {
  const int rc = rt_pack_scene(d, budget, &g[k]);
  const RtRefitPlan& p = g[k].plan;
  sizes[0] = g[k].blob.size(), sizes[1] = g[k].flag_geo.size(), sizes[2] = p.height_nodes.size(), sizes[3] = p.height_offset.size();
  sizes[4] = p.thr_src.size(), sizes[5] = p.recv_cell.size(), sizes[6] = p.tri_slot.size(), sizes[7] = p.mat_class.size();
  return rc;
}
void probe_get(int k, unsigned char* blob, float* geo, uint32_t* dev, uint32_t* misc, float* aabb) {
  static_assert(sizeof(RtDevScene) == 8 + 19 * 4 + 4, "RtDevScene changed: update this probe and DEV_FIELDS");
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

// ---- the device state: ONE uploaded scene, every part in an allocation of its own ------------------------------------------
namespace {
struct DevState {
  int slot = -1;           // the slot it was uploaded from
  RtPackedScene up;        // ... as it was then
  char* blob = nullptr;
  float* geo = nullptr;    // null when the scene has no receiver cells (RtUpdateArgs::flag_geo)
  uint32_t* plan[4] = {nullptr, nullptr, nullptr, nullptr};  // height_nodes, thr_src, recv_cell, tri_slot
  float* bounds = nullptr; // 8 words, zeroed: lo, hi, bits(receivers disabled), 0
  bool bounds_live = false;  // a geometry delta ran: as rt_update.cpp, bounds and counter are only read after one
} D;
hipStream_t stream = nullptr;
uint32_t launches = 0;
int dead = 0;  // the first HIP error, sticky: nothing further is started on the device after it
#define TRY(x)                                                 \
  do {                                                         \
    const hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return dead = 1000 + (int)e_;        \
  } while (0)

int to_device(void** dst, const void* src, size_t bytes) {
  *dst = nullptr;
  if (!bytes) return 0;
  TRY(hipMalloc(dst, bytes));
  TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
int release() {
  if (dead) return dead;
  void* p[7] = {D.blob, D.geo, D.plan[0], D.plan[1], D.plan[2], D.plan[3], D.bounds};
  for (void* q : p)
    if (q) TRY(hipFree(q));
  D = DevState();
  return 0;
}
}  // namespace

extern "C" {
int probe_release() {
  const int rc = release();
  if (rc == 0 && stream) {
    TRY(hipStreamDestroy(stream));
    stream = nullptr;
  }
  return rc;
}
int probe_upload(int k) {
  int rc = release();
  if (rc) return rc;
  TRY(hipSetDevice(0));
  if (!stream) TRY(hipStreamCreate(&stream));
  const RtPackedScene& s = g[k];
  const std::vector<uint32_t>* parts[4] = {&s.plan.height_nodes, &s.plan.thr_src, &s.plan.recv_cell, &s.plan.tri_slot};
  if ((rc = to_device((void**)&D.blob, s.blob.data(), s.blob.size()))) return rc;
  if ((rc = to_device((void**)&D.geo, s.flag_geo.data(), s.flag_geo.size() * 4))) return rc;
  for (int i = 0; i < 4; i++)
    if ((rc = to_device((void**)&D.plan[i], parts[i]->data(), parts[i]->size() * 4))) return rc;
  TRY(hipMalloc((void**)&D.bounds, 32));
  TRY(hipMemset(D.bounds, 0, 32));
  D.slot = k, D.up = s;
  return 0;
}
int probe_update_device(int k, const rt_scene_delta* h) {
  if (dead) return dead;
  if (k != D.slot) return -100;
  const RtPackedScene& s = g[k];
  int rc = rt_check_scene_delta(s.dev, s.plan, h, h ? h->materials : nullptr);
  if (rc != RT_OK) return rc;
  const size_t ns = s.dev.n_spheres, nt = h->tri_count, nm = s.plan.mat_class.size(), nl = s.dev.n_lights;
  rt_scene_delta d = *h;
  void* tmp[8];
  int n = 0;
#define STAGE(member, floats)                                                          \
  if (h->member) {                                                                     \
    if ((rc = to_device(&tmp[n], h->member, (size_t)(floats) * 4))) return rc;         \
    d.member = (const float*)tmp[n++];                                                 \
  }
  STAGE(sphere_center, 3 * ns) STAGE(sphere_r_sq, ns)
  if (h->sphere_center) d.sphere_r_inv = d.sphere_r_sq;  // (present, never read: as rt_update.cpp)
  STAGE(tri_v1, 3 * nt) STAGE(tri_e1, 3 * nt) STAGE(tri_e2, 3 * nt) STAGE(tri_normal, 3 * nt)
  STAGE(materials, nm * RT_MATERIAL_STRIDE) STAGE(lights, nl * RT_LIGHT_STRIDE)
#undef STAGE
  RtUpdateArgs u{};
  u.base = D.blob, u.flag_geo = D.geo;
  u.height_nodes = D.plan[0], u.thr_src = D.plan[1], u.recv_cell = D.plan[2], u.tri_slot = D.plan[3];
  u.bounds = D.bounds;
  u.height_offset = s.plan.height_offset.data();
  u.n_heights = s.plan.height_offset.empty() ? 0u : (uint32_t)s.plan.height_offset.size() - 1u;
  u.n_materials = (uint32_t)nm;
  launches = 0;
  TRY((hipError_t)rt_launch_update(s.dev, u, d, stream, &launches));
  TRY(hipStreamSynchronize(stream));
  if (d.sphere_center || d.tri_count) D.bounds_live = true;
  for (int i = 0; i < n; i++)
    if (tmp[i]) TRY(hipFree(tmp[i]));
  return 0;
}
uint32_t probe_launches() { return launches; }
int probe_download(int j) {
  if (dead) return dead;
  if (D.slot < 0) return -100;
  RtPackedScene out = D.up;
  if (!out.blob.empty()) TRY(hipMemcpy(out.blob.data(), D.blob, out.blob.size(), hipMemcpyDeviceToHost));
  if (!out.flag_geo.empty()) TRY(hipMemcpy(out.flag_geo.data(), D.geo, out.flag_geo.size() * 4, hipMemcpyDeviceToHost));
  float b[8];
  TRY(hipMemcpy(b, D.bounds, 32, hipMemcpyDeviceToHost));
  if (D.bounds_live) {
    memcpy(out.aabb_lo, b, 12), memcpy(out.aabb_hi, b + 3, 12);
    memcpy(&out.plan.receivers_disabled, b + 6, 4);
  }
  g[j] = out;
  return 0;
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("update_kernels_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    # none of the csrc sources: the packer, the host model and the kernels come from the library under test
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src),
                          "-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    lib.probe_launches.restype = C.c_uint32
    lib._sizes, lib._creation = {}, {}
    yield lib
    lib.probe_release()


# ---- driving the probe -------------------------------------------------------------------------------------------------------
def hip_ok(rc, what):
    assert rc == 0, f"{what}: " + (f"hipError_t {rc - HIP_ERROR}" if rc >= HIP_ERROR else f"code {rc}")


def creation(probe, name, flat):
    """slot 0 := the packed creation state of a named scene (packed once per module, kept in slots 3..7)"""
    if name not in probe._creation:
        k = 3 + len(probe._creation)
        assert k < 8
        pack(probe, k, flat)
        probe._creation[name] = k
    k = probe._creation[name]
    probe.probe_copy(k, 0)
    probe._sizes[0] = probe._sizes[k]
    return get(probe, 0, flat)


def upload(probe, k=0):
    hip_ok(probe.probe_upload(k), "probe_upload")
    probe._uploaded = k


def host_copy(probe, k=0, to=2):
    probe.probe_copy(k, to)
    probe._sizes[to] = probe._sizes[k]


def update_device(probe, old, new, full=False, groups=None):
    """old -> new on the device state; the same delta refit() of the host file builds"""
    groups = groups or _abi.scene_delta_groups(old, new, full=full)
    d, keep = _abi.make_scene_delta(new, groups)
    return probe.probe_update_device(probe._uploaded, C.byref(d))


def download(probe, flat, j=1):
    hip_ok(probe.probe_download(j), "probe_download")
    probe._sizes[j] = probe._sizes[probe._uploaded]
    return get(probe, j, flat)


def both(probe, old, new, full=False, groups=None, nan_ok=False, what=""):
    """one delta on the device state (read back into slot 1) and on the host model in slot 2; compared; -> (device, host)"""
    hip_ok(update_device(probe, old, new, full, groups), f"{what}: probe_update_device")
    assert refit(probe, 2, old, new, full, groups) == 0, probe.probe_error()
    dev, host = download(probe, new), get(probe, 2, new)
    dev.exempted = assert_device_equals_host(dev, host, nan_ok, what)
    return dev, host


# ---- the comparison ----------------------------------------------------------------------------------------------------------
# per section: words of a record, and which of them are floats (the only places the both-NaN exemption can apply)
RECORDS = {"off_spheres": (4, (0, 1, 2, 3)), "off_sphere_rad": (1, (0,)), "off_sphere_mat": (1, ()), "off_tri_isect": (12, tuple(range(12))),
           "off_recv": (12, tuple(range(8))), "off_srecv": (2, ()), "off_tri_shade": (4, (0, 1, 2)), "off_tri_id": (1, ()),
           "off_nodes": (16, (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)), "off_nodes_oct": (16, (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)),
           "off_nodes_thr": (8, (0, 1, 2, 4, 5, 6)), "off_materials": (12, tuple(range(12))), "off_lights": (8, tuple(range(8)))}
assert set(RECORDS) == set(LAYOUT)


def float_words(p):
    m = np.zeros(len(p.blob) // 4, bool)
    size = record_bytes(p)
    for off, (words, floats) in RECORDS.items():
        n = size[off] // (4 * words)
        m[p.dev[off] // 4:p.dev[off] // 4 + n * words].reshape(n, words)[:, list(floats)] = True
    return m


def where(p, w):
    """word w of the blob, named: section, record, word of the record"""
    size = record_bytes(p)
    off = max((o for o in LAYOUT if p.dev[o] <= 4 * w), key=lambda o: p.dev[o])
    words = RECORDS[off][0]
    rel = w - p.dev[off] // 4
    if 4 * rel >= size[off]:
        return f"slack behind {off}, word {rel - size[off] // 4}"
    return f"{off} record {rel // words} word {rel % words}"


def is_nan(w):
    return (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def assert_device_equals_host(dev, host, nan_ok=False, what=""):
    """every word of the blob, every word of flag_geo, the six bounds, receivers_disabled; -> the words exempted (both NaN)"""
    assert dev.dev == host.dev and len(dev.blob) == len(host.blob) and len(dev.blob) % 4 == 0, what
    a, b = dev.blob.view(np.uint32), host.blob.view(np.uint32)
    diff = a != b
    exempted = 0
    if nan_ok and diff.any():
        both_nan = diff & float_words(host) & is_nan(a) & is_nan(b)  # (so the host word IS a NaN wherever the exemption is used)
        exempted = int(both_nan.sum())
        diff &= ~both_nan
    if diff.any():
        w = np.flatnonzero(diff)
        lines = [f"{where(host, int(i))}: device {int(a[i]):#010x}, host {int(b[i]):#010x}" for i in w[:6]]
        raise AssertionError(f"{what}: {len(w)} words of the blob differ\n  " + "\n  ".join(lines))
    ga, gb = dev.geo.view(np.uint32), host.geo.view(np.uint32)
    assert len(ga) == len(gb), what
    if not np.array_equal(ga, gb):
        i = int(np.flatnonzero(ga != gb)[0])
        raise AssertionError(f"{what}: flag_geo triangle {i // 12} word {i % 12}: device {int(ga[i]):#010x}, host {int(gb[i]):#010x}")
    ba, bb = dev.aabb.view(np.uint32), host.aabb.view(np.uint32)
    assert np.array_equal(ba, bb), f"{what}: bounds: device {dev.aabb} ({ba}), host {host.aabb} ({bb})"
    assert dev.receivers_disabled == host.receivers_disabled, f"{what}: receivers_disabled: device {dev.receivers_disabled}, host {host.receivers_disabled}"
    return exempted


def expected_launches(p, plan, groups):
    """the launches of one delta as DESIGN.md 6c lists them: one per non-empty height, nothing for a group that is absent"""
    d, n = p.dev, 0
    n += bool(groups["spheres"] and d["n_spheres"])
    if groups["triangles"]:
        n += 2 + int((np.diff(plan["height_offset"].astype(np.int64)) > 0).sum()) + 1 + bool(d["n_thr"])
    if groups["spheres"] or groups["triangles"]:
        n += 1 + bool(d["n_triangles"])
    n += bool(groups["materials"] and len(plan["mat_class"])) + bool(groups["lights"] and d["n_lights"])
    return n


# ---- scenes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat_scene(name):
    return SCENES[name]()


MOVABLE = sorted(set(SCENES) - {"empty"})


def soup(n, seed=40):
    """n small triangles in the unit cube"""
    r = np.random.default_rng(seed + n)
    v1, e1, e2 = r.uniform(0.1, 0.9, (n, 3)), r.normal(0, 0.2, (n, 3)), r.normal(0, 0.2, (n, 3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * n, mats=[MAT_DIFFUSE], lights=[LIGHT]).contiguous()


def sphere_field(n, seed=21):
    """n spheres in [2, 8]^3 -- every coordinate of every extent positive, so no -0.0 reaches fminf -- and one triangle"""
    r = np.random.default_rng(seed)
    tri = dict(v1=[[4, 4, 4]], e1=[[1, 0, 0.5]], e2=[[0, 1, 0.5]], nrm=[[0, 0, 1]], tm=[0]) if n > 3 else {}
    return flat_of(sc=r.uniform(2, 8, (n, 3)), sr_sq=r.uniform(0.01, 0.04, n), sm=np.arange(n) % 2, mats=[MAT_DIFFUSE, MAT_DIFFUSE],
                   lights=[LIGHT], **tri).contiguous()


def with_spheres(flat, centre, r_sq=None):
    r_sq = flat.sphere_r_sq if r_sq is None else np.asarray(r_sq, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_inv = (F32(1) / np.sqrt(np.abs(r_sq))).astype(F32)
    return cases.copy(flat, sphere_center=np.asarray(centre, F32), sphere_r_sq=r_sq, sphere_r_inv=r_inv)


def extremes_moved(flat, amount, who=None):
    """the spheres that carry the six bounds (or `who`: six indices, lo x y z then hi x y z) pushed `amount` outwards"""
    c = flat.sphere_center.astype(np.float64)
    r = np.sqrt(np.abs(flat.sphere_r_sq.astype(np.float64)))
    who = who or [int(np.argmin(c[:, a] - r)) for a in range(3)] + [int(np.argmax(c[:, a] + r)) for a in range(3)]
    for k, i in enumerate(who):
        c[i, k % 3] = (c[:, k % 3].min() - amount) if k < 3 else (c[:, k % 3].max() + amount)
    return with_spheres(flat, c), who


# ---- a. every edit the host file checks ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("edit", ["turn", "jitter", "spheres_lights_material"])
@pytest.mark.parametrize("name", MOVABLE)
def test_device_equals_the_host_model_and_a_fresh_pack(probe, name, edit):
    t0 = time.perf_counter()
    flat = flat_scene(name)
    new = edits(name, flat)[edit]
    a = creation(probe, name, flat)
    upload(probe)
    host_copy(probe)
    dev, host = both(probe, flat, new, what=f"{name} / {edit}")
    assert not np.array_equal(dev.blob, a.blob), "the edit changes the scene"
    # the device against the independent reference directly, not only through the shared header
    check_against_fresh(probe, a, dev, new)
    check_tree(dev, new)
    print(f"{name} / {edit}: {len(dev.blob)} bytes, {probe.probe_launches()} launches, {time.perf_counter() - t0:.2f} s")


# ---- b. identity -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", MOVABLE)
def test_restating_the_creation_arrays_changes_no_device_byte(probe, name):
    flat = flat_scene(name)
    a = creation(probe, name, flat)
    upload(probe)
    host_copy(probe)
    dev, host = both(probe, flat, flat, full=True, what=f"{name} / identity")
    assert_device_equals_host(dev, a, what=f"{name} / identity against the upload")
    assert dev.receivers_disabled == 0
    groups = _abi.scene_delta_groups(flat, flat, full=True)
    assert probe.probe_launches() == expected_launches(a, plan_of(probe, 0), groups)


# ---- c. a sequence on one device state -------------------------------------------------------------------------------------------
def far_away(flat, rng, distance):
    """triangles [first, first + count) translated by `distance` scene diagonals along z: their receiver maps lose their
    conditioning against the scene bounds (err * R <= 0.04, rt_upd_recv)"""
    return cases.turn_mesh(flat, rng, 0.0, (0.0, 0.0, distance * cases.diagonal(flat)))


FAR = 10.0  # scene diagonals: chosen on the CPU so that some receivers of the mesh fail the bound and some hold (asserted)


def receiver_steps(name="semesterbild"):
    flat = flat_scene(name)
    first, count = cases.mesh_range(name, flat)
    far = far_away(flat, (first, count), FAR)
    victim = first + count // 2
    degenerate = cases.copy(flat, tri_e2=np.where(np.arange(flat.n_triangles)[:, None] == victim, F32(2) * flat.tri_e1, flat.tri_e2).astype(F32))
    return flat, count, victim, [("far away", far), ("one zero-area triangle", degenerate), ("back", flat)]


def test_receiver_case_is_neither_vacuous_nor_total(probe):
    """host-side precondition of (c) and (g): the middle step disables some receivers of the mesh, not all of them"""
    flat, count, victim, steps = receiver_steps()
    a = creation(probe, "semesterbild", flat)
    host_copy(probe)
    prev, counters = flat, []
    for label, step in steps:
        assert refit(probe, 2, prev, step) == 0, probe.probe_error()
        counters.append(get(probe, 2, step).receivers_disabled)
        prev = step
    print(f"receivers disabled: {counters} of {count} mesh triangles")
    assert 0 < counters[0] < count
    assert section(a, "off_recv", flat.n_triangles, 12)[victim, 8] != 0 and counters[1] == 1, "nn == 0 takes exactly the one triangle's cells"
    assert counters[2] == 0


@gpu
def test_a_sequence_of_updates_on_one_device_state(probe):
    """the scripted animation, a step that disables receivers, and back: the blob is carried on the device from step to
    step without another upload, the host model alongside"""
    name = "semesterbild"
    flat = flat_scene(name)
    a = creation(probe, name, flat)
    upload(probe)
    host_copy(probe)
    frames = cases.animation(name, flat)
    assert len(frames) >= 6 and frames[-1][1] is flat
    far = far_away(frames[-2][1], cases.mesh_range(name, flat), FAR)
    prev, counters = flat, []
    for label, step in frames[:-1] + [("far away", far), frames[-1]]:
        dev, host = both(probe, prev, step, what=f"sequence / {label}")
        counters.append(host.receivers_disabled)
        prev = step
    assert counters[-2] > 0 and counters[-1] == 0, "the counter rises and comes back down"
    assert_device_equals_host(dev, a, what="sequence: back at the creation blob")
    print(f"receivers disabled along the sequence: {counters}")


# ---- d. partial triangle ranges at the launch-shape edges ------------------------------------------------------------------------
def partial_ranges(flat):
    first, count = cases.mesh_range("semesterbild", flat)
    return {"first": (first, 1), "last": (flat.n_triangles - 1, 1), "255": (first + 3, 255), "256": (first + 3, 256), "257": (first + 3, 257),
            "whole": (first, count)}


@gpu
@pytest.mark.parametrize("which", ["first", "last", "255", "256", "257", "whole"])
def test_partial_triangle_range_touches_only_its_triangles_on_the_device(probe, which):
    flat = flat_scene("semesterbild")
    first, count = partial_ranges(flat)[which]
    assert first + count <= flat.n_triangles
    new = cases.turn_mesh(flat, (first, count), 35.0)
    assert _abi.scene_delta_groups(flat, new)["triangles"] == (first, count)
    a = creation(probe, "semesterbild", flat)
    upload(probe)
    host_copy(probe)
    dev, host = both(probe, flat, new, what=f"range ({first}, {count})")
    # directly: the records of every other triangle are the uploaded ones
    t = section(a, "off_tri_id", a.dev["n_slots"], 1)[:, 0] & IDX
    other = (t < first) | (t >= first + count)
    n_slots, nt = a.dev["n_slots"], flat.n_triangles
    assert np.array_equal(section(dev, "off_tri_isect", n_slots, 12)[other], section(a, "off_tri_isect", n_slots, 12)[other])
    assert np.array_equal(section(dev, "off_tri_shade", n_slots, 4)[other], section(a, "off_tri_shade", n_slots, 4)[other])
    outside = np.ones(nt, bool)
    outside[first:first + count] = False
    assert np.array_equal(section(dev, "off_tri_shade", n_slots + nt, 4)[n_slots:][outside], section(a, "off_tri_shade", n_slots + nt, 4)[n_slots:][outside])
    assert np.array_equal(dev.geo.view(np.uint32).reshape(nt, 12)[outside], a.geo.view(np.uint32).reshape(nt, 12)[outside])
    assert not np.array_equal(section(dev, "off_tri_isect", n_slots, 12)[~other], section(a, "off_tri_isect", n_slots, 12)[~other])


# ---- e. the smallest trees ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_smallest_trees(probe, n):
    flat = flat_scene("one_triangle") if n == 1 else soup(n)
    a = pack(probe, 0, flat)
    nodes = section(a, "off_nodes", a.dev["n_nodes"], 16)
    absent = sum(c == EMPTY for nd in nodes for _, _, c, _ in children(nd))
    print(f"{n} triangles: {a.dev['n_nodes']} nodes, {absent} absent children, {a.dev['n_thr']} threaded entries")
    if n == 1:
        assert a.dev["n_nodes"] == 1 and absent == 1, "a single leaf beside an absent child"
    upload(probe)
    host_copy(probe)
    dev, host = both(probe, flat, flat, full=True, what=f"{n} triangles / identity")
    assert_device_equals_host(dev, a, what=f"{n} triangles / identity against the upload")
    new = cases.jitter(flat, 0.05)
    dev, host = both(probe, flat, new, what=f"{n} triangles / jitter")
    check_against_fresh(probe, a, dev, new)  # (check_tree within: an absent child keeps its NaN box)


@gpu
def test_every_height_of_a_deep_tree_is_its_own_small_launch(probe):
    """text_lowres: more heights than 256-thread workgroups in any of them, so the ordering between parents and children
    rests on the launch boundaries alone"""
    name = "semesterbild"
    flat = flat_scene(name)
    a = creation(probe, name, flat)
    plan = plan_of(probe, 0)
    per_height = np.diff(plan["height_offset"].astype(np.int64))
    assert len(per_height) > int(np.ceil(per_height / 256).max()) and (per_height > 0).all()
    upload(probe)
    host_copy(probe)
    new = cases.jitter(flat, 0.05)
    groups = _abi.scene_delta_groups(flat, new)
    dev, host = both(probe, flat, new, what="deep tree / jitter")
    assert probe.probe_launches() == expected_launches(a, plan, groups) == 2 + len(per_height) + 4
    nodes = check_tree(dev, new)
    assert np.array_equal(section(dev, "off_nodes_oct", 8 * len(nodes), 16), expected_octants(nodes))
    assert np.array_equal(section(dev, "off_nodes_thr", dev.dev["n_thr"], 8), expected_threaded(nodes))
    print(f"{len(per_height)} heights of {per_height.tolist()} nodes")


# ---- f. the bounds kernel's stride loop and reduction ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1100, 3])
def test_bounds_reduction_equals_the_host_loop(probe, n):
    """1100 spheres: a thread of the one 1024-thread workgroup visits two; 3 spheres and nothing else: most threads reduce
    +-INFINITY.  The spheres that carry the bounds move out, then others take over"""
    flat = sphere_field(n)
    assert (flat.sphere_center - np.sqrt(flat.sphere_r_sq)[:, None] > 1).all()
    a = pack(probe, 0, flat)
    upload(probe)
    host_copy(probe)
    who = [1099, 1029, 5, 1024, 700, 1098] if n > 1024 else [0, 1, 2, 2, 0, 1]
    out, who = extremes_moved(flat, 1.0, who)
    dev, host = both(probe, flat, out, what=f"{n} spheres / extremes out")
    c, r = out.sphere_center.astype(np.float64), np.sqrt(out.sphere_r_sq.astype(np.float64))
    assert [int(np.argmin(c[:, k] - r)) for k in range(3)] + [int(np.argmax(c[:, k] + r)) for k in range(3)] == who
    assert not np.array_equal(dev.aabb, a.aabb) and np.array_equal(dev.aabb, expected_bounds(out))
    mid = c.copy()
    mid[who] = 5.0  # the six go to the middle: other spheres carry the bounds
    back = with_spheres(out, mid)
    dev2, host = both(probe, out, back, what=f"{n} spheres / extremes in")
    assert not np.array_equal(dev2.aabb, dev.aabb)
    assert np.array_equal(dev2.aabb, expected_bounds(back))
    for upd, new in ((dev, out), (dev2, back)):  # (slot 2 is free now: the fresh packs go there)
        if n > 3:
            check_against_fresh(probe, a, upd, new)
        else:  # (no tree to check)
            fresh = pack(probe, 2, new)
            assert np.array_equal(upd.aabb, fresh.aabb)
            for off, words in (("off_spheres", 4), ("off_sphere_rad", 1)):
                assert np.array_equal(section(upd, off, n, words), section(fresh, off, n, words)), off


# ---- g. receivers disabled and restored ------------------------------------------------------------------------------------------
@gpu
def test_receivers_are_disabled_and_restored_on_the_device(probe):
    flat, count, victim, steps = receiver_steps()
    a = creation(probe, "semesterbild", flat)
    upload(probe)
    host_copy(probe)
    prev, counters = flat, []
    for label, step in steps:
        dev, host = both(probe, prev, step, what=f"receivers / {label}")
        r_dev, r_host = (section(x, "off_recv", flat.n_triangles, 12) for x in (dev, host))
        assert np.array_equal(r_dev[:, 8], r_host[:, 8]), "the R words"
        assert dev.receivers_disabled == int(((section(a, "off_recv", flat.n_triangles, 12)[:, 8] != 0) & (r_dev[:, 8] == 0)).sum())
        counters.append(dev.receivers_disabled)
        prev = step
    assert 0 < counters[0] < count and counters[1] == 1 and counters[2] == 0, counters
    assert_device_equals_host(dev, a, what="receivers: back at the creation blob")


# ---- h. the float sequences at their edges ---------------------------------------------------------------------------------------
N_EDGE = 4096


def edge_scene():
    """4096 spheres, 4096 triangles, 4096 material rows; every triangle uses row 0, whose transmissive class the deltas keep"""
    r = np.random.default_rng(31)
    n = N_EDGE
    v1, e1, e2 = r.uniform(1, 3, (n, 3)), r.normal(0, 0.05, (n, 3)), r.normal(0, 0.05, (n, 3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mats = np.tile(np.array(MAT_DIFFUSE, F32), (n, 1))
    mats[:, 5] = r.uniform(1, 2, n)
    return flat_of(sc=r.uniform(1, 3, (n, 3)), sr_sq=np.full(n, 1e-4), sm=np.arange(n), v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * n, mats=mats,
                   lights=[LIGHT]).contiguous()


def random_floats(r, n):
    """random bit patterns: every exponent, either sign, infinities and NaNs among them"""
    return r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F32)


def subnormals(r, n):
    return (r.integers(1, 1 << 23, n).astype(np.uint32) | (r.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(F32)


def log_uniform(r, shape, lo, hi):
    with np.errstate(over="ignore", under="ignore"):
        return (np.power(10.0, r.uniform(lo, hi, shape)) * r.choice([-1.0, 1.0], shape)).astype(F32)


def edge_materials(flat):
    r = np.random.default_rng(32)
    one = F32(1)
    fixed = np.array([1, -1, 0.0, -0.0, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), -np.nextafter(one, F32(2)), -np.nextafter(one, F32(0)),
                      np.inf, -np.inf, np.nan, np.finfo(F32).max, np.finfo(F32).tiny, 2.0 ** -149], F32)
    huge = (r.uniform(2.0 ** 126, 2.0 ** 128 * (1 - 2.0 ** -24), 256) * r.choice([-1.0, 1.0], 256)).astype(F32)  # 1 / ior subnormal
    ior = np.concatenate([fixed, subnormals(r, 512), huge, random_floats(r, N_EDGE)])[:N_EDGE]
    m = flat.materials.copy()
    m[:, 5] = ior
    return cases.copy(flat, materials=m)


def edge_spheres(flat):
    r = np.random.default_rng(33)
    fixed = np.array([0.0, np.finfo(F32).max, -np.finfo(F32).max, np.inf, -np.inf, np.nan, -1.0, -1e-4, np.finfo(F32).tiny, 2.0 ** -149], F32)
    r_sq = np.concatenate([fixed, subnormals(r, 1024), -r.uniform(0, 4, 512).astype(F32), log_uniform(r, 1024, -44, 38.5), random_floats(r, N_EDGE)])[:N_EDGE]
    c = flat.sphere_center.copy()
    c[100, 0], c[101, 1], c[102, 2] = np.inf, -np.inf, np.nan
    return with_spheres(flat, c, r_sq)


def edge_triangles(flat, tiny):
    """tiny = False: every component of either edge log-uniform in 1e-30 .. 1e30, so the six products of X underflow,
    overflow and meet as inf - inf.  tiny = True: edges of 1e-45 .. 1e-20, subnormal floats among them: a cross product far
    below fp32 (its components are exact differences of exact fp64 products, multiples of 2^-298 when they do not vanish, so
    fp64 itself never goes subnormal here), nn down to 1e-180, map words that overflow fp32 or land among its subnormals"""
    r = np.random.default_rng(35 if tiny else 34)
    n = flat.n_triangles
    e1, e2 = (log_uniform(r, (n, 3), -45, -20) if tiny else log_uniform(r, (n, 3), -30, 30) for _ in range(2))
    if tiny:
        e2[::7] = (e1[::7] * F32(2)).astype(F32)  # parallel (a doubling is exact): nn == 0
    v1 = flat.tri_v1.copy()
    v1[200, 0], v1[201, 1], v1[202, 2] = np.inf, np.nan, -np.inf
    e1[203, 0], e2[204, 1] = np.nan, np.inf
    return cases.copy(flat, tri_v1=v1, tri_e1=e1, tri_e2=e2)


def scaled_triangles(flat):
    """the creation triangles shrunk about their first vertices by powers of two down to 2^-40: fp64 map words of up to 1e13,
    and with v1 of order 1 translation words that leave fp32's range in neither direction -- finite maps, live bound"""
    r = np.random.default_rng(36)
    s = np.exp2(-r.integers(0, 41, (flat.n_triangles, 1))).astype(F32)
    return cases.copy(flat, tri_e1=(flat.tri_e1 * s).astype(F32), tri_e2=(flat.tri_e2 * s).astype(F32))


def is_subnormal(x):
    w = np.ascontiguousarray(x).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return (w > 0) & (w < 0x00800000)


def edge_steps():
    flat = edge_scene()
    s1 = edge_materials(flat)
    s2 = edge_spheres(s1)
    s3 = edge_triangles(s2, tiny=False)
    s4 = edge_triangles(with_spheres(s3, flat.sphere_center, flat.sphere_r_sq), tiny=True)
    s5 = scaled_triangles(cases.copy(s4, tri_v1=flat.tri_v1, tri_e1=flat.tri_e1, tri_e2=flat.tri_e2))
    return flat, [("ior", s1), ("r_sq", s2), ("edges 1e-30 .. 1e30", s3), ("edges 1e-45 .. 1e-20", s4), ("edges shrunk", s5)]


def assert_edge_classes(a, label, host):
    """what the host model's output must contain for the step to be the test it is meant to be"""
    nt = N_EDGE
    if label == "ior":
        q = section(host, "off_materials", N_EDGE, 12, F32)
        assert is_subnormal(q[:, 9]).sum() >= 50 and np.isinf(q[:, 9]).sum() >= 50 and np.isnan(q[:, 10]).any() and np.isinf(q[:, 10]).any()
        assert is_subnormal(q[:, 10]).any() or (q[:, 10] == 0).any()
    if label == "r_sq":
        rad = section(host, "off_sphere_rad", N_EDGE, 1, F32)[:, 0]
        assert is_subnormal(section(host, "off_spheres", N_EDGE, 4, F32)[:, 3]).sum() >= 1000 and np.isinf(rad).any() and np.isnan(rad).any()
        assert np.isfinite(host.aabb).all(), "the bounds ignore what is not finite"
    if label.startswith("edges 1e-30"):
        x = section(host, "off_tri_isect", nt, 12, F32)[:, 9:12]
        assert np.isnan(x).sum() >= 10 and np.isinf(x).any() and (is_subnormal(x).any() or (x == 0).any()), "a NaN X: inf - inf"
        assert np.isfinite(host.aabb).all()
        q = section(host, "off_recv", nt, 12)[:, :8]
        assert is_subnormal(q).sum() >= 10 and np.isinf(q.view(F32)).any(), "fp64 -> fp32 among the subnormals and beyond FLT_MAX"
    if label.startswith("edges 1e-45"):
        r_new, r_old = section(host, "off_recv", nt, 12), section(a, "off_recv", nt, 12)
        bad_map = ~np.isfinite(r_new[:, :8].view(F32)).all(1)
        assert ((r_old[:, 8] != 0) & bad_map & (r_new[:, 8] == 0)).sum() >= 10, "an R forced to 0 by a map word that is not finite"
        assert (r_new[::7, :8] == 0).all(), "nn == 0: no maps"
    if label == "edges shrunk":
        r_new, r_old = section(host, "off_recv", nt, 12), section(a, "off_recv", nt, 12)
        q = r_new[:, :8].view(F32)
        assert np.isfinite(q).all() and (np.abs(q) > 1e9).any()
        assert 0 < host.receivers_disabled < int((r_old[:, 8] != 0).sum()), "the conditioning bound decides, either way"


def test_float_edge_inputs_reach_every_class(probe):
    """host-side precondition of (h), without a GPU: a subnormal and an infinite q[9], a NaN X, an R forced to 0 by a map
    word that is not finite -- and every delta passes rt_check_scene_delta"""
    flat, steps = edge_steps()
    a = pack(probe, 0, flat)
    assert a.n_tri_cells > 0 and (section(a, "off_recv", N_EDGE, 12)[:, 8] > 1).sum() > N_EDGE // 2
    host_copy(probe)
    prev = flat
    for label, step in steps:
        assert refit(probe, 2, prev, step) == 0, probe.probe_error()
        assert_edge_classes(a, label, get(probe, 2, step))
        prev = step


@gpu
def test_float_sequences_at_their_edges(probe):
    flat, steps = edge_steps()
    a = pack(probe, 0, flat)
    upload(probe)
    host_copy(probe)
    prev = flat
    for label, step in steps:
        dev, host = both(probe, prev, step, nan_ok=True, what=f"edges / {label}")
        assert_edge_classes(a, label, host)
        print(f"edges / {label}: equal; {dev.exempted} words NaN on both sides with different bits; {host.receivers_disabled} receivers disabled")
        prev = step


# ---- i. refusals reach no kernel -------------------------------------------------------------------------------------------------
@gpu
def test_a_refused_delta_reaches_no_kernel(probe):
    flat = flat_scene("mesh_with_glass")
    a = creation(probe, "mesh_with_glass", flat)
    upload(probe)
    host_copy(probe)
    moved = cases.recolour(cases.move_spheres(cases.jitter(flat, 0.05)))
    everything = _abi.scene_delta_groups(flat, moved, full=True)
    glass_made_opaque = moved.materials.copy()
    glass_made_opaque[1, 6], glass_made_opaque[1, 8] = 0.0, 1.0
    refusals = {"a partial group": lambda d: setattr(d, "tri_e1", None),
                "a range beyond n_triangles": lambda d: setattr(d, "tri_first", 1),
                "a changed transmissive class": lambda d: setattr(d, "materials", glass_made_opaque.ctypes.data)}
    for what, change in refusals.items():
        d, keep = _abi.make_scene_delta(moved, everything)
        change(d)
        rc_host = probe.probe_refit(2, C.byref(d))
        msg = probe.probe_error()
        rc = probe.probe_update_device(0, C.byref(d))
        assert rc == rc_host == _abi.RT_ERR_INVALID_ARG and probe.probe_error() == msg, (what, rc, rc_host, msg)
        assert_device_equals_host(download(probe, flat), a, what=f"{what}: the device state after the refusal")
    # ... and the same delta unchanged is taken
    dev, host = both(probe, flat, moved, full=True, what="the delta the refusals were made from")
    assert not np.array_equal(dev.blob, a.blob)
