"""Scenes, probes and references for the direct tests of rt_flags_kernel (csrc/rt_kernels.hip), the first of the three
once-per-scene stages behind the per-cell shadow candidate lists:

  slots the literal triangle test accepts for some shadow ray from the cell
    <=  slots rt_flags_kernel lists (or its bit says "not clear")
    <=  slots the float64 restatement of the fat-beam rule (f64_fat_beam.py) does not clearly reject

The scenes, the hull, the shadow rays and the literal test are those of test_cell_prune_host.py; the scenes added here aim at
the stage's own rules.  Every scene is packed with the budget of test_cell_prune_gpu.py (at most 4096 receiver cells), on the
CPU and on the GPU alike, so that cell numbers mean the same in both.  reference() is computed once per scene and shared by
every test of a run; nothing in it calls the kernel."""
import ctypes as C
import dataclasses
import os
import subprocess
import tempfile

import numpy as np

import f64_fat_beam as fb
import test_cell_prune_host as host
from test_cell_prune_host import CASES, EPS, F32, _soup, flat_of, hit_points, hull_of, light_points, literal, load, shadow_rays, soft_cfg  # noqa: F401
from test_scene_pack_host import CSRC, HIPCC, ROOT, ptr

END, OVERFLOW = host.END, host.OVERFLOW
ALL_CELLS_UP_TO = 512  # scenes of at most this many cells: every active cell is checked, not only the ones load() selects
NEAR_CAP = 0.02        # share of the rejected triples that may fall in the near band, per scene


# ---- scenes --------------------------------------------------------------------------------------------------------------------
FLOOR = ([0, 0, 0], [1, 0, 0], [0, 1, 0])
_COL = [1.0, 0.9, 0.8, 3.0]


def _behind_and_through_quads():
    c30, s30 = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    c100, s100 = np.cos(np.radians(100.0)), np.sin(np.radians(100.0))
    a, b = 0.02 * np.array([c30, 0.0, s30]), np.array([0.0, 0.02, 0.0])
    return [FLOOR,
            ([0.2, 0.2, -1e-4], [0.3, 0, 0], [0, 0.3, 0]),                 # 1e-4 below the floor: behind the surface
            ([1, 0, 0], [0.5, 0, 0], [0, 1, 0]),                           # coplanar with the floor, beside it
            (np.array([0.62, 0.61, 0.0]) - 0.5 * a - 0.5 * b, a, b),       # crosses the floor plane at 30 degrees inside one cell
            ([0, 0, 0], [0, 1, 0], [0.5 * c100, 0, 0.5 * s100]),           # a wall meeting the floor at 100 degrees along x = 0
            # a long strip 0.02 above the floor under the low third light, its v1 far away: it shadows the rim of a cell whose
            # centre it misses, and |v1 - p| is many times the distance to the light (delta * B is what keeps it)
            ([-0.5, 0.81, 0.02], [0.83, 0, 0], [0, 0.004, 0])]


def _transformed(flat, scale=1.0, shift=(0.0, 0.0, 0.0)):
    shift = np.asarray(shift, np.float64)
    lights = flat.lights.astype(np.float64).copy()
    lights[:, :3] = lights[:, :3] * scale + shift
    return dataclasses.replace(flat, tri_v1=(flat.tri_v1.astype(np.float64) * scale + shift).astype(F32), tri_e1=(flat.tri_e1 * F32(scale)).astype(F32),
                               tri_e2=(flat.tri_e2 * F32(scale)).astype(F32), lights=lights.astype(F32)).contiguous()


def behind_and_through_scene(n_lights=3):
    lights = [[0.5, 0.5, 0.6], [1.2, 0.2, 0.3], [0.3, 0.8, 0.04], [0.63, 0.6, 0.05], [1.4, 0.9, 0.8], [-0.05, 0.5, 0.3], [0.3, 0.3, 0.02], [0.9, 0.1, 1.5]]
    return _soup(_behind_and_through_quads(), lights=[p + _COL for p in lights[:n_lights]])


def grazing_scene():
    """a light 2e-3 above the floor plane off to one side (dseg.z ~ 0 for every floor cell: inv.z is clamped), a low fence
    between it and the floor, and a light 2e-4 above the floor whose cloud ball straddles the floor, placed so that the ball's
    centre lies over the centre of a cell (the floor has 22 x 22 of them), closer to it than beam_delta"""
    quads = [FLOOR, ([1.1, 0.3, -0.01], [0, 0.4, 0], [0, 0, 0.03]), ([0.3, 0.45, 0.0005], [0.05, 0, 0.002], [0, 0.1, 0])]
    return _soup(quads, lights=[[1.3, 0.5, 2e-3] + _COL, [0.4758, 0.4758, 2e-4] + _COL])


def sphere_edges_scene():
    """two receiver spheres (radius 0.2 and 0.01) over a floor, panes over a cube-map face centre (+z), a face edge (+x/+z) and
    a face corner (+x/+y/+z) of the large one with a light behind each, a pane tangent to it within 1e-4, and a third small
    sphere as an occluder between a light and the floor"""
    ctr, rad = np.array([0.5, 0.5, 0.5]), 0.2

    def pane(direction, dist, half):
        d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
        a = np.cross(d, [0.0, 1.0, 0.0] if abs(d[1]) < 0.9 else [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(d, a)
        return (ctr + d * dist - half * a - half * b, 2 * half * a, 2 * half * b)

    quads = [FLOOR, pane([0, 0, 1], 0.3, 0.04), pane([1, 0, 1], 0.3, 0.04), pane([1, 1, 1], 0.3, 0.04),
             ([0.5 - rad - 1e-4, 0.4, 0.4], [0, 0.2, 0], [0, 0, 0.2])]
    spheres = [(0.5, 0.5, 0.5, rad), (1.1, 0.3, 0.3, 0.01), (0.2, 0.9, 0.3, 0.03)]
    lights = [list(ctr + np.array(d) / np.linalg.norm(d) * 0.7) + _COL for d in ([0, 0, 1], [1, 0, 1], [1, 1, 1])] + [[0.05, 0.5, 0.5] + _COL]
    return _soup(quads, spheres=spheres, lights=lights)


RAGGED_CELLS = 257


def ragged_scene():
    """257 receiver cells: two quads of 64 cells per triangle, a degenerate triangle without any (R == 0) and, after it, a small
    one with a single cell (R == 1) that also sets the scene's size.  257 % 64 == 1: the last workgroup of rt_flags_kernel holds
    one lane, its wavefront 63 lanes without a cell"""
    flat = _soup([FLOOR, ([0.05, 0.1, 0.35], [1, 0, 0], [0, 0.8, 0])], lights=[[0.5, 0.5, 1.1] + _COL, [1.2, -0.2, 0.25] + _COL])
    v1 = np.array([[0.7, 0.2, 0.1], [1.6, 1.0, 0.9]], F32)
    e1 = np.array([[0.1, 0.0, 0.0], [0.01, 0.0, 0.0]], F32)
    e2 = np.array([[0.05, 0.0, 0.0], [0.0, 0.01, 0.0]], F32)  # (the first one has e2 = e1 / 2: no area, R == 0)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], F32)
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])  # noqa: E731
    return dataclasses.replace(flat, tri_v1=cat(flat.tri_v1, v1), tri_e1=cat(flat.tri_e1, e1), tri_e2=cat(flat.tri_e2, e2),
                               tri_normal=cat(flat.tri_normal, nrm), tri_material=cat(flat.tri_material, np.zeros(2, np.uint32))).contiguous()


def known_answers_scene():
    """a unit floor, a 0.1 x 0.1 opaque quad at height 0.3 over its middle, one light at (0.5, 0.5, 0.9)"""
    return _soup([FLOOR, ([0.45, 0.45, 0.3], [0.1, 0, 0], [0, 0.1, 0])], lights=[[0.5, 0.5, 0.9] + _COL])


# name -> (cfg, flat, every n-th cell), as test_cell_prune_host.CASES
NEW = {
    "behind_and_through": lambda: (soft_cfg(), behind_and_through_scene(), None),
    "grazing": lambda: (soft_cfg(), grazing_scene(), None),
    "far_and_tiny_far": lambda: (soft_cfg(), _transformed(behind_and_through_scene(), shift=(1000.0, -1000.0, 1000.0)), None),
    "far_and_tiny_tiny": lambda: (soft_cfg(), _transformed(behind_and_through_scene(), scale=1e-3), None),
    "sphere_edges": lambda: (soft_cfg(), sphere_edges_scene(), None),
    "eight_lights": lambda: (soft_cfg(), behind_and_through_scene(8), None),
    "ragged": lambda: (soft_cfg(), ragged_scene(), None),
    "known_answers": lambda: (soft_cfg(), known_answers_scene(), None),       # 23 x 23 cells on the floor
    "known_answers_fine": lambda: (soft_cfg(), known_answers_scene(), None),  # 89 x 89
}
KNOWN = ["known_answers", "known_answers_fine"]
REUSED = ["synthetic", "far_side", "sliver", "sphere_receiver", "semesterbild"]
SCENES = REUSED + [n for n in NEW if not n.startswith("known_answers")]
for _name, _make in NEW.items():
    host.CASES.setdefault(_name, _make)


def budget_of(name, flat):
    """the flags' input and at most 4096 cells (test_cell_prune_gpu.py); ragged: exactly 257; known_answers_fine: at most 16384
    (89 x 89 cells on the floor)"""
    return 48 * flat.n_triangles + (2 * RAGGED_CELLS if name == "ragged" else 32768 if name == "known_answers_fine" else 8192)


# ---- host probe: the one of test_cell_prune_host.py and the beam constants ---------------------------------------------------------
HOST_EXTRA = r'''
extern "C" {
// rt_beam_constants: out = beam_delta, beam_delta_e5, beam_eps_push, beam_eps_ulp, beam_eps_o
void probe_beam(float eps, float cloud_delta, float* out) {
  RtDevParams P{};
  P.cloud_delta = cloud_delta;
  rt_beam_constants(eps, &P);
  out[0] = P.beam_delta, out[1] = P.beam_delta_e5, out[2] = P.beam_eps_push, out[3] = P.beam_eps_ulp, out[4] = P.beam_eps_o;
}
}
'''

# the GPU probe: built and linked as test_cell_prune_gpu.py's (against the built librt_hip.so: the kernel driven is the one that ships)
GPU_PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <cstring>
#include "rt_scene_pack.h"
static RtPackedScene g;
static int dead = 0;  // the first HIP error, sticky: nothing further is started on the device after it
#define TRY(x)                                                 \
  do {                                                         \
    const hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return dead = 1000 + (int)e_;        \
  } while (0)
extern "C" {
const char* probe_error() { return rt_last_error(); }
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint32_t* out) {
  const int rc = rt_pack_scene(d, budget, &g);
  out[0] = g.n_cells, out[1] = g.n_tri_cells, out[2] = g.dev.n_lights, out[3] = g.dev.n_slots;
  return rc;
}
// flags and lists of the packed scene for one light-cloud table, as rt_flags_kernel leaves them; with_lists = 0: no lists
// (cell_list_out = nullptr), raw_lists is not written
int probe_flags(const float* cloud, uint64_t n_floats, const float* f, float eps, int with_lists, uint16_t* raw_lists, uint16_t* raw_flags) {
  if (dead) return dead;
  if (!g.n_cells || g.dev.n_lights > 8u || g.dev.n_slots > 65533u) return -100;
  std::vector<float> scaled;
  float ball[4];
  rt_scale_cloud(cloud, n_floats, f, &scaled, ball);
  RtDevParams P{};
  memcpy(P.cloud_centre, ball, 12);
  P.cloud_delta = ball[3];
  P.eps_distance = eps;
  rt_beam_constants(eps, &P);
  P.cand_cap = 64u;
  const size_t list_bytes = (size_t)g.n_cells * g.dev.n_lights * 16u, flag_bytes = (size_t)g.n_cells * 2u;
  char* blob = nullptr;
  float* geo = nullptr;
  uint16_t *lists = nullptr, *flags = nullptr;
  TRY(hipSetDevice(0));
  TRY(hipMalloc((void**)&blob, g.blob.size()));
  TRY(hipMalloc((void**)&geo, g.flag_geo.size() * 4));
  TRY(hipMalloc((void**)&lists, list_bytes + 64));
  TRY(hipMalloc((void**)&flags, flag_bytes + 64));
  TRY(hipMemcpy(blob, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice));
  TRY(hipMemcpy(geo, g.flag_geo.data(), g.flag_geo.size() * 4, hipMemcpyHostToDevice));
  TRY(hipMemset(lists, 0xFF, list_bytes));
  TRY(hipMemset(flags, 0, flag_bytes));
  RtDevScene sc = g.dev;
  sc.base = blob;
  P.flag_out = flags, P.flag_geo = (const float4*)geo, P.cell_list_out = with_lists ? lists : nullptr;
  P.n_cells = g.n_cells, P.n_tri_cells = g.n_tri_cells;
  TRY((hipError_t)rt_launch_flags(sc, P, nullptr));
  TRY(hipDeviceSynchronize());
  if (with_lists) TRY(hipMemcpy(raw_lists, lists, list_bytes, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(raw_flags, flags, flag_bytes, hipMemcpyDeviceToHost));
  TRY(hipFree(blob));
  TRY(hipFree(geo));
  TRY(hipFree(lists));
  TRY(hipFree(flags));
  return 0;
}
}
'''

_built = {}


def _compile(tag, source, extra):
    if tag not in _built:
        d = tempfile.mkdtemp(prefix=f"flags_{tag}_probe_")
        src, so = os.path.join(d, "probe.cpp"), os.path.join(d, "probe.so")
        with open(src, "w") as fh:
            fh.write(source)
        out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                              "-I", os.path.join(ROOT, "include"), "-shared", "-o", so, src] + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lib = C.CDLL(so)
        lib.probe_error.restype = C.c_char_p
        _built[tag] = lib
    return _built[tag]


def have_hipcc():
    return os.path.exists(HIPCC)


def host_probe():
    return _compile("host", host.PROBE + HOST_EXTRA, [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp", "rt_cell_prune.cpp")])


def gpu_probe():
    from hslu_i.ba_raytracing.f2501_raytracer_amd import _lib
    lib_dir, lib_name = os.path.split(os.path.abspath(_lib.LIB_PATH))
    return _compile("gpu", GPU_PROBE, ["-L", lib_dir, f"-l:{lib_name}", f"-Wl,-rpath,{lib_dir}"])


def run_flags(gpu, k, with_lists=1):
    """rt_flags_kernel on the scene of case k -> (raw_lists [n_cells, n_lights, 8] or None, raw_flags [n_cells])"""
    from hslu_i.ba_raytracing.f2501_raytracer_amd import sampling
    out = np.zeros(4, np.uint32)
    assert gpu.probe_pack(C.byref(k.desc), C.c_uint64(k.budget), ptr(out)) == 0, gpu.probe_error()
    assert [int(v) for v in out] == [k.n_cells, k.n_tri_cells, k.dev["n_lights"], k.dev["n_slots"]], "the GPU probe packed the scene the host probe packed"
    cs = np.ascontiguousarray(sampling.cloud_sets(k.cfg), F32)
    f = np.array([k.cfg.fw, k.cfg.fh, k.cfg.fd], F32)
    lists = np.zeros((k.n_cells, k.dev["n_lights"], 8), np.uint16)
    flags = np.zeros(k.n_cells, np.uint16)
    rc = gpu.probe_flags(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(k.cfg.eps_distance), C.c_int(with_lists), ptr(lists), ptr(flags))
    assert rc == 0, f"probe_flags: {rc}"
    return (lists if with_lists else None), flags


# ---- a scene, packed on the host, with everything the references need -------------------------------------------------------------
_cases = {}


def case(name):
    """load() of test_cell_prune_host.py with the 4096-cell budget, plus the beam constants, the slots' boxes, the spheres and
    the hull of every cell that is checked.  The probe holds one packed scene: probe_* calls are only valid until the next case()"""
    if name in _cases:
        return _cases[name]
    probe = host_probe()
    flat = host.CASES[name]()[1]
    k = _cases[name] = load(probe, name, budget_of(name, flat))
    k.budget = budget_of(name, flat)
    assert 0 < k.n_cells <= (16384 if name == "known_answers_fine" else 4096), k.n_cells
    out = np.zeros(5, F32)
    probe.probe_beam(C.c_float(k.cfg.eps_distance), C.c_float(k.cloud_delta), ptr(out))
    assert out[0] == k.beam_delta and out[4] == k.eps_o
    k.consts = fb.Consts(out[0], out[2], out[3], out[4], k.centre)
    ns = k.dev["n_slots"]
    q = k.isect.astype(np.float64)
    corners = np.stack([q[:, 0:3], q[:, 0:3] + q[:, 3:6], q[:, 0:3] + q[:, 6:9]], 1)
    k.slot_lo, k.slot_hi = corners.min(1), corners.max(1)
    nsph = k.dev["n_spheres"]
    o = k.dev["off_spheres"]
    k.spheres = k.blob[o:o + 16 * nsph].view(F32).reshape(nsph, 4).copy()  # centre, r^2
    o = k.dev["off_sphere_rad"]
    k.sphere_rad = k.blob[o:o + 4 * nsph].view(F32).copy()                 # (upper bound of the radius)
    k.hulls = {c: hull_of(probe, c) for c in range(k.n_cells)}  # (None: the cell is never looked up)
    k.active = np.array([k.hulls[c] is not None for c in range(k.n_cells)])
    k.checked = [c for c in (range(k.n_cells) if k.n_cells <= ALL_CELLS_UP_TO else k.cells) if k.active[c]]
    lo = np.minimum(k.slot_lo.min(0), (k.spheres[:, :3] - k.sphere_rad[:, None]).min(0)) if nsph else k.slot_lo.min(0)
    hi = np.maximum(k.slot_hi.max(0), (k.spheres[:, :3] + k.sphere_rad[:, None]).max(0)) if nsph else k.slot_hi.max(0)
    k.scene_size = float(np.linalg.norm(hi - lo))
    assert ns == len(k.isect)
    return k


# ---- the sphere literal test, float32 ----------------------------------------------------------------------------------------------
def sphere_literal(sph, o, d):
    """sphere_intersect of oracle/rt_oracle.c (no culling) on float32 arrays, operation for operation -> (hit, t);
    sph = centre[3], r^2"""
    f = host._dot_fused
    v = (o - sph[0:3]).astype(F32)
    b = (F32(2) * f(d, v)).astype(F32)
    cc = (f(v, v) - sph[3]).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        disc = (b.astype(np.float64) * b.astype(np.float64) + (F32(-4) * cc).astype(F32).astype(np.float64)).astype(F32)  # fmaf(b, b, -4 cc)
        ok = disc >= 0
        sq = np.sqrt(np.where(ok, disc, F32(0))).astype(F32)
        mba, sa = (-b * F32(0.5)).astype(F32), (sq * F32(0.5)).astype(F32)
        t0, t1 = (mba - sa).astype(F32), (mba + sa).astype(F32)
        t0v, t1v = t0 >= 0, t1 >= 0
        use0 = t0v & (~t1v | (t0 < t1))
        use1 = t1v & ~use0
    return ok & (use0 | use1), np.where(use0, t0, t1).astype(F32)


# ---- the references of a scene: what the literal tests accept and what the f64 rule says, per (cell, light) -----------------------
class Ref:
    pass


_refs = {}


def beam_of(k, c, l, **ablation):
    pm, pt = k.hulls[c]
    return fb.cell_beam(k.consts, pm, pt, k.lights[l], **ablation)


F64_ALL_CELLS_UP_TO_SLOTS = 256  # scenes of at most this many leaf slots: the f64 verdicts are taken for EVERY active cell
BUSY_CELLS = 48                  # ... and the cells with the most candidates by them get the literal test too
SPHERE_CELLS = 48


def reference(name, seed=1):
    """-> Ref with, per checked (cell, light): accepted (slots the literal test accepts for some shadow ray) and sphere_hit
    (some shadow ray meets some sphere); per (cell, light) of R.f64_cells (every active cell of a small scene): rejected /
    clear (the f64 rule's verdict on every slot) and the sphere verdicts.  R.checked: the cells load() selects (every active
    one of a scene of at most 512 cells), an even spread of the sphere cells and the cells the f64 rule keeps most for"""
    if name in _refs:
        return _refs[name]
    k = case(name)
    rng = np.random.default_rng(seed)
    R = Ref()
    R.k, R.accepted, R.sphere_hit, R.rejected, R.clear, R.sph = k, {}, {}, {}, {}, {}
    R.rays = R.offered = 0
    R.sample_rays, R.sample_sphere_rays = [], []
    pad = 1e-3 * k.scene_size
    nl = k.dev["n_lights"]
    n_cloud = len(k.cloud)
    checked = set(k.checked)
    sphere_cells = [c for c in range(k.n_tri_cells, k.n_cells) if k.active[c]]
    all_cells = k.dev["n_slots"] <= F64_ALL_CELLS_UP_TO_SLOTS
    checked |= set(sphere_cells[::max(1, len(sphere_cells) // (SPHERE_CELLS if all_cells else SPHERE_CELLS // 8))])
    R.f64_cells = [c for c in range(k.n_cells) if k.active[c]] if all_cells else sorted(checked)
    busy = {}
    for c in R.f64_cells:
        for l in range(nl):
            B = beam_of(k, c, l)
            R.rejected[c, l], R.clear[c, l] = fb.triangles(B, k.isect)
            R.sph[c, l] = fb.spheres(B, k.spheres[:, :3], k.sphere_rad)
            busy[c] = busy.get(c, 0) + int((~R.clear[c, l]).sum()) + 8 * int((R.rejected[c, l] & ~R.clear[c, l]).sum())
    if all_cells:
        checked |= set(sorted(busy, key=lambda c: (-busy[c], c))[:BUSY_CELLS])
    R.checked = sorted(checked)
    for c in R.checked:
        pm, pt = k.hulls[c]
        h = hit_points(rng, pm, pt)
        for l in range(nl):
            B = beam_of(k, c, l)
            # every slot whose box meets the padded box of hull + light ball (a literal hit has t <= tmax: it lies in that convex set)
            ball = np.stack([B.c - k.consts.beam_delta, B.c + k.consts.beam_delta])
            lo, hi = np.minimum(pt.min(0), ball[0]) - pad, np.maximum(pt.max(0), ball[1]) + pad
            offered = np.nonzero(((k.slot_lo <= hi) & (k.slot_hi >= lo)).all(1))[0]
            cloud_pts = (k.lights[l][None] + k.cloud).astype(F32)
            so0, d0, tmax0 = shadow_rays(h, cloud_pts, k.cfg.eps_distance)
            acc_slots = set()
            for s in offered:
                extra = light_points(k, l, pm.astype(np.float64), k.isect[s])[n_cloud:]
                so1, d1, tmax1 = shadow_rays(h, extra, k.cfg.eps_distance)
                so, d, tmax = np.concatenate([so0, so1]), np.concatenate([d0, d1]), np.concatenate([tmax0, tmax1])
                valid, t = literal(k.isect[s], so, d)
                R.rays += len(so)
                if (valid & (t <= tmax)).any():
                    acc_slots.add(int(s))
                if len(R.sample_rays) < 64 and rng.random() < 0.05:
                    i = int(rng.integers(len(so)))
                    R.sample_rays.append((int(s), so[i].copy(), d[i].copy(), bool(valid[i]), float(t[i])))
            R.offered += len(offered)
            R.accepted[c, l] = acc_slots
            hit_any = False
            for i, sph in enumerate(k.spheres):
                # the cloud's points and the ball's extremes towards and away from the sphere, and sideways
                w = sph[:3].astype(np.float64) - B.c
                dirs = [w, np.cross(w, B.dseg), np.cross(np.cross(w, B.dseg), B.dseg)]
                ext = [B.c + sg * k.consts.beam_delta * v / np.linalg.norm(v) for v in dirs if np.linalg.norm(v) > 0 for sg in (1.0, -1.0)]
                so, d, tmax = so0, d0, tmax0
                if ext:
                    so1, d1, tmax1 = shadow_rays(h, np.asarray(ext, F32), k.cfg.eps_distance)
                    so, d, tmax = np.concatenate([so0, so1]), np.concatenate([d0, d1]), np.concatenate([tmax0, tmax1])
                hit, t = sphere_literal(sph, so, d)
                hit_any |= bool((hit & (t <= tmax)).any())
                if len(R.sample_sphere_rays) < 64 and rng.random() < 0.2:
                    j = int(rng.integers(len(so)))
                    R.sample_sphere_rays.append((i, so[j].copy(), d[j].copy(), bool(hit[j]), float(t[j])))
            R.sphere_hit[c, l] = hit_any
    _refs[name] = R
    return R


def unsound(R, rejected_clear=None):
    """the (cell, light, slot) the literal test accepts and the f64 rule clearly rejects (none, if the rule is sound)"""
    clear = rejected_clear or R.clear
    return [(c, l, s) for (c, l), acc in R.accepted.items() for s in sorted(acc) if clear[c, l][s]]


def near_share(R):
    """-> (rejected triples, of them in the near band)"""
    rej = sum(int(v.sum()) for v in R.rejected.values())
    near = sum(int((R.rejected[key] & ~R.clear[key]).sum()) for key in R.rejected)
    return rej, near


# ---- the shape of raw lists and flags (every cell of a scene) -----------------------------------------------------------------------
def check_shape(lists, flags, n_slots, active=None):
    """what rt_flags_kernel may leave behind: inactive cells untouched (flags 0, lists all 0xFFFF), lists of distinct slots
    < n_slots padded with 0xFFFF, 0xFFFE only ever in entry 0, and (given flags) bit l set <=> list l empty"""
    lists = np.asarray(lists)
    n_cells, nl, _ = lists.shape
    assert nl <= 8 and n_slots <= OVERFLOW
    over = lists[:, :, 0] == OVERFLOW
    assert not (lists[:, :, 1:] == OVERFLOW).any(), "0xFFFE only ever in entry 0"
    body = np.where(over[:, :, None], END, lists)   # (what follows the mark of an overflowed list is not read)
    filled = body != END
    assert (body[filled] < n_slots).all(), "listed slots exist"
    assert not (filled[:, :, 1:] & ~filled[:, :, :-1]).any(), "0xFFFF only after the last entry"
    srt = np.sort(body, axis=2)
    assert not ((srt[:, :, 1:] == srt[:, :, :-1]) & (srt[:, :, 1:] != END)).any(), "listed slots are distinct"
    empty = lists[:, :, 0] == END
    if active is None and flags is not None:  # (an active cell whose lists are all empty has their bits set: its word is not 0)
        active = ~((np.asarray(flags) == 0) & empty.all(1))
    if active is not None:
        assert (lists[~active] == END).all(), "inactive cells keep lists of all 0xFFFF"
        if flags is not None:
            assert (np.asarray(flags)[~active] == 0).all(), "inactive cells have flags 0"
    if flags is not None:
        bits = ((np.asarray(flags)[:, None] >> np.arange(nl)[None, :]) & 1).astype(bool)
        sel = slice(None) if active is None else active
        assert np.array_equal(bits[sel], empty[sel]), "bit l is set <=> list l is empty"
        assert (np.asarray(flags) >> 8 >> nl == 0).all() and ((np.asarray(flags) & 0xFF) >> nl == 0).all(), "no bit beyond the scene's lights"
    return int(filled.sum()), int(over.sum())


# ---- receiver_cell of rt_kernels.hip, float32 ---------------------------------------------------------------------------------------
def _fma(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def receiver_cell(k, prim, p):
    """the receiver cell of the hit point p (float32[3]) of primitive `prim` (spheres first, then triangles) as the render
    looks it up, from the packed blob: off_recv rows, off_srecv, the cube-map face rule; None = no cell"""
    ns = k.dev["n_spheres"]
    p = np.asarray(p, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if prim >= ns:
            o = k.dev["off_recv"] + (prim - ns) * 48
            ru, rv = k.blob[o:o + 16].view(F32), k.blob[o + 16:o + 32].view(F32)
            R, first = (int(v) for v in k.blob[o + 32:o + 40].view(np.uint32))
            if R == 0:
                return None
            Rf = F32(R)
            cu = F32(F32(_fma(ru[0], p[0], _fma(ru[1], p[1], F32(ru[2] * p[2]))) + ru[3]) * Rf)
            cv = F32(F32(_fma(rv[0], p[0], _fma(rv[1], p[1], F32(rv[2] * p[2]))) + rv[3]) * Rf)
            ci, cj = int(min(max(cu, F32(0)), F32(Rf - F32(1)))), int(min(max(cv, F32(0)), F32(Rf - F32(1))))
            return first + ci + R * cj if ci + cj < R else None
        o = k.dev["off_srecv"] + prim * 8
        Rs, first = (int(v) for v in k.blob[o:o + 8].view(np.uint32))
        if Rs == 0:
            return None
        dd = (p - k.spheres[prim, :3]).astype(F32)
        ax, ay, az = np.abs(dd)
        mx = bool(ax >= ay and ax >= az)
        my = bool(not mx and ay >= az)
        dm, du, dv = (dd[0], dd[1], dd[2]) if mx else ((dd[1], dd[2], dd[0]) if my else (dd[2], dd[0], dd[1]))
        face = (0 if mx else (2 if my else 4)) + (1 if dm < 0 else 0)
        inv, Rf = F32(F32(1) / max(abs(dm), F32(1e-30))), F32(Rs)
        ci = int(min(max(F32(F32(_fma(du, inv, F32(1)) * F32(0.5)) * Rf), F32(0)), F32(Rf - F32(1))))
        cj = int(min(max(F32(F32(_fma(dv, inv, F32(1)) * F32(0.5)) * Rf), F32(0)), F32(Rf - F32(1))))
        return first + (face * Rs + cj) * Rs + ci


def outside_hull(pm, pt, p):
    """how far p lies outside the hull of the 8 points pt (a parallelogram taken twice, or a frustum), <= 0: inside"""
    pt, p = pt.astype(np.float64), np.asarray(p, np.float64)
    if np.array_equal(pt[:4], pt[4:]):
        a, b = pt[1] - pt[0], pt[2] - pt[0]
        n = np.cross(a, b)
        n /= np.linalg.norm(n)
        coef = np.linalg.lstsq(np.stack([a, b, n], 1), p - pt[0], rcond=None)[0]
        la, lb = np.linalg.norm(a), np.linalg.norm(b)
        return max(-coef[0] * la, (coef[0] - 1) * la, -coef[1] * lb, (coef[1] - 1) * lb, abs(coef[2]))
    mid = pt.mean(0)
    worst = -np.inf
    for f in ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (1, 3, 7, 5), (3, 2, 6, 7), (2, 0, 4, 6)):
        q = pt[list(f)]
        n = np.cross(q[2] - q[0], q[3] - q[1])
        n /= np.linalg.norm(n)
        if n @ (mid - q.mean(0)) > 0:
            n = -n
        worst = max(worst, float(n @ (p - q.mean(0))))
    return worst
