"""The rule that thins out the per-cell shadow candidate lists (csrc/rt_cell_prune.h) checked on the CPU, through its host
model (rt_cell_prune_cell / rt_cell_prune_packed, csrc/rt_cell_prune.cpp -- the same functions the kernel is made of),
compiled host-only with a probe, as the packer is in test_scene_pack_host.py.

Soundness, zero tolerance: a pruned (cell, light, triangle) must not be accepted by the literal triangle test for ANY shadow
ray the render can cast from the cell towards the light's cloud.  The probe offers EVERY leaf slot of the scene to every
tested (cell, light) as a candidate (in lists of 8), which is more than rt_flags_kernel would ever list.  Of the pruned
triples the test takes every one the weaker rule (no far side, products of 1-norms) keeps -- the marginal ones, up to a cap --
and a seeded sample of the rest, builds the shadow rays as shadow_geom does in float32 (hit point -> light sample, origin
pushed by eps along the re-normalised direction, tmax = |lp - so|; the two fused dot products of its length are taken in
float64 and rounded) from

  hit points:   the 8 points of the cell's enlarged hull, its centre, the centre pushed off the surface both ways by the
                rounding of o + t d (4e-7 |p|_1), and random points of the hull
  light points: every point of every cloud set (light + scaled offset, float32), and the extremes of the ball of radius
                beam_delta about the cloud's centre along +-w, +-w_c and +-X

and runs the oracle's literal triangle test (rt_oracle.c: triangle_intersect, restated in float32 numpy and held to
rt_oracle_triangle on a sample of the same rays) on each: none may be accepted with EPS < t <= tmax."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import material_cases as mc
import oracle_lib
import scene_update_cases as cases
from test_scene_pack_host import CSRC, DEV_FIELDS, HIPCC, IDX, MAT_DIFFUSE, MAT_GLASS, ROOT, flat_of, ptr
from hslu_i.ba_raytracing.f2501_raytracer_amd import RenderConfig, _abi, sampling

F32 = np.float32
EPS = F32(1.1920929e-7)
FAR, EUCLID, NO_RHO_WC, NO_RHO_FAR = 1, 2, 4, 8
FULL, WEAK = FAR | EUCLID, 0
END, OVERFLOW = 0xFFFF, 0xFFFE

PROBE = r'''
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>
#include "rt_cell_prune.h"
#include "rt_scene_pack.h"
static RtPackedScene g;
static RtCellPruneArgs A;
extern "C" {
int probe_pack(const rt_scene_desc* d, uint64_t budget, uint64_t* sizes) {
  const int rc = rt_pack_scene(d, budget, &g);
  sizes[0] = g.blob.size(), sizes[1] = g.flag_geo.size(), sizes[2] = g.n_cells, sizes[3] = g.n_tri_cells;
  return rc;
}
void probe_get(unsigned char* blob, uint32_t* dev) {
  static_assert(sizeof(RtDevScene) == 8 + 19 * 4 + 4, "RtDevScene changed: update this probe and DEV_FIELDS");
  if (!g.blob.empty()) memcpy(blob, g.blob.data(), g.blob.size());
  memcpy(dev, &g.dev.off_spheres, 19 * 4);
}
// the constants of a frame: the scaled cloud table and (out) cloud centre[3], cloud_delta, beam_delta, beam_eps_o
void probe_consts(const float* cloud, uint64_t n_floats, const float* f, float eps, float* scaled, float* out) {
  std::vector<float> s;
  float ball[4];
  rt_scale_cloud(cloud, n_floats, f, &s, ball);
  memcpy(scaled, s.data(), s.size() * 4);
  RtDevParams P{};
  P.cloud_delta = ball[3];
  rt_beam_constants(eps, &P);
  A = RtCellPruneArgs();
  A.flag_geo = g.flag_geo.data();
  A.n_cells = g.n_cells, A.n_tri_cells = g.n_tri_cells;
  memcpy(A.cloud_centre, ball, 12);
  A.beam_delta = P.beam_delta, A.beam_eps_o = P.beam_eps_o;
  memcpy(out, ball, 16);
  out[4] = P.beam_delta, out[5] = P.beam_eps_o;
}
// the hull of cell c as the rule sees it: out = pm[3], pt[8][3]; returns whether the cell is ever looked up
int probe_hull(uint32_t c, float* out) {
  float pm[3], pt[8][3], extra;
  if (!rt_prune_cell_hull(g.dev, (const char*)g.blob.data(), A, c, pm, pt, &extra)) return 0;
  memcpy(out, pm, 12), memcpy(out + 3, pt, 96);
  return 1;
}
// every leaf slot offered to cell c as a candidate, 8 at a time: pruned[l * n_slots + slot] = 1 when the rule removes it
void probe_prune_all(uint32_t c, uint32_t mode, uint8_t* pruned) {
  RtCellPruneArgs a = A;
  a.mode = mode;
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  alignas(16) uint16_t list[8 * RT_PRUNE_LIST_SLOTS];
  for (uint32_t s0 = 0; s0 < ns; s0 += RT_PRUNE_LIST_SLOTS) {
    for (uint32_t l = 0; l < nl; l++)
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS; k++) list[l * RT_PRUNE_LIST_SLOTS + k] = s0 + k < ns ? (uint16_t)(s0 + k) : (uint16_t)RT_PRUNE_LIST_END;
    uint16_t flag = 0;
    rt_cell_prune_cell(g.dev, (const char*)g.blob.data(), a, c, list, &flag);
    for (uint32_t l = 0; l < nl; l++) {
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS && s0 + k < ns; k++) pruned[(size_t)l * ns + s0 + k] = 1;
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS; k++) {
        const uint16_t s = list[l * RT_PRUNE_LIST_SLOTS + k];
        if (s < RT_PRUNE_LIST_OVERFLOW) pruned[(size_t)l * ns + s] = 0;
      }
    }
  }
}
// probe_prune_all over many cells, on up to 16 threads, for the rule `mode`, the weak rule (0) and the full rule:
// totals = {triples tested, pruned by `mode`, pruned by the weak rule, pruned by the weak rule but not by the full one};
// marginal: the {cell, light, slot} pruned by `mode` and kept by the weak rule, others: every `every`-th (by a hash) of the rest
// of the pruned ones; both capped at `cap` triples, *n_marginal / *n_others count them all the same
void probe_scan(const uint32_t* cells, uint32_t n, uint32_t mode, uint64_t* totals, uint32_t* marginal, uint64_t* n_marginal, uint32_t* others,
                uint64_t* n_others, uint64_t cap, uint32_t every) {
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::mutex mu;
  std::atomic<uint32_t> next{0};
  totals[0] = totals[1] = totals[2] = totals[3] = 0, *n_marginal = *n_others = 0;
  auto work = [&]() {
    std::vector<uint8_t> pm((size_t)nl * ns), pw((size_t)nl * ns), pf((size_t)nl * ns);
    std::vector<uint32_t> mine, rest;
    uint64_t t[4] = {0, 0, 0, 0};
    for (uint32_t i; (i = next++) < n;) {
      const uint32_t c = cells[i];
      float o[27];
      if (!probe_hull(c, o)) continue;
      probe_prune_all(c, mode, pm.data()), probe_prune_all(c, 0u, pw.data());
      if (mode == RT_PRUNE_FULL) pf = pm; else probe_prune_all(c, RT_PRUNE_FULL, pf.data());
      for (uint32_t l = 0; l < nl; l++)
        for (uint32_t s = 0; s < ns; s++) {
          const size_t k = (size_t)l * ns + s;
          t[0]++, t[1] += pm[k], t[2] += pw[k], t[3] += pw[k] && !pf[k];
          if (pm[k] && !pw[k]) mine.insert(mine.end(), {c, l, s});
          else if (pm[k] && (c * 2654435761u + l * 40503u + s * 97u) % every == 0u) rest.insert(rest.end(), {c, l, s});
        }
    }
    std::lock_guard<std::mutex> lock(mu);
    for (int k = 0; k < 4; k++) totals[k] += t[k];
    for (size_t k = 0; k + 2 < mine.size(); k += 3, ++*n_marginal)
      if (*n_marginal < cap) memcpy(marginal + 3 * *n_marginal, &mine[k], 12);
    for (size_t k = 0; k + 2 < rest.size(); k += 3, ++*n_others)
      if (*n_others < cap) memcpy(others + 3 * *n_others, &rest[k], 12);
  };
  std::vector<std::thread> th;
  for (unsigned k = 0; k < nt; k++) th.emplace_back(work);
  for (auto& x : th) x.join();
}
// the host model on whole arrays ([n_cells][n_lights][8] and [n_cells]), in place
void probe_prune_lists(uint32_t mode, uint16_t* lists, uint16_t* flags, uint32_t n_cells) {
  RtCellPruneArgs a = A;
  a.mode = mode, a.lists = lists, a.flags = flags, a.n_cells = n_cells;
  rt_cell_prune_packed(g, a);
}
const char* probe_error() { return rt_last_error(); }
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cell_prune_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src)] +
                         [os.path.join(CSRC, f) for f in ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp", "rt_cell_prune.cpp")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def soft_cfg():
    return RenderConfig.from_features(["anti_aliasing", "soft_shadows"], n_cloud_sets=64)


def _quad(v, a, b):
    """two triangles of the parallelogram v, v + a, v + b, v + a + b -> (v1, e1, e2) rows"""
    v, a, b = (np.asarray(x, np.float64) for x in (v, a, b))
    return [v, v + a + b], [a, -a], [b, -b]


def _soup(quads, spheres=(), lights=()):
    v1, e1, e2 = [], [], []
    for q in quads:
        a, b, c = _quad(*q)
        v1 += a
        e1 += b
        e2 += c
    nrm = np.cross(np.asarray(e1), np.asarray(e2))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    sc = [s[:3] for s in spheres]
    return flat_of(sc=sc, sr_sq=[s[3] ** 2 for s in spheres], sm=[0] * len(sc), v1=v1, e1=e1, e2=e2, nrm=nrm, tm=[0] * len(v1),
                   mats=[MAT_DIFFUSE, MAT_GLASS], lights=lights).contiguous()


def far_side_scene():
    """a floor, a light 0.2 above it, and two panes BEHIND the light (seen from the floor), tilted so that their boxes reach
    down over the light: the beam's box test keeps them.  The first lies 1e-3 behind the light's position -- inside its cloud
    (the offsets reach 2.9e-3), so some sample rays do reach it and nothing may remove it; the second lies 8e-3 behind,
    beyond every sample, and only the far-side inequality can remove it"""
    light = [0.5, 0.5, 0.2, 1.0, 0.9, 0.8, 3.0]
    tilt = 0.3
    pane = lambda dz: ([0.2, 0.2, 0.2 + dz - 0.3 * tilt], [0.6, 0.0, 0.6 * tilt], [0.0, 0.6, 0.0])  # noqa: E731  z = 0.2 + dz + tilt (x - 0.5)
    return _soup([([0, 0, 0], [1, 0, 0], [0, 1, 0]), pane(1e-3), pane(8e-3)], lights=[light, [0.1, 0.9, 0.6, 0.2, 0.3, 0.4, 1.5]])


def sliver_scene():
    """a floor and, between it and the lights, slivers: edges nearly parallel (|X| tiny against |e1||e2|), one of them long"""
    quads = [([0, 0, 0], [1, 0, 0], [0, 1, 0])]
    flat = _soup(quads, lights=[[0.5, 0.5, 0.4, 1.0, 0.9, 0.8, 3.0], [0.9, 0.1, 0.15, 0.2, 0.3, 0.4, 1.5]])
    v1 = np.array([[0.3, 0.3, 0.2], [0.1, 0.6, 0.1], [0.45, 0.5, 0.3]], F32)
    e1 = np.array([[0.4, 0.1, 0.02], [0.8, -0.3, 0.05], [0.1, 0.0, 0.0]], F32)
    e2 = (e1 * F32(0.7) + np.array([[1e-4, -2e-4, 1e-4], [0, 1e-5, 0], [0, 1e-3, 0]], F32)).astype(F32)
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])  # noqa: E731
    return dataclasses.replace(flat, tri_v1=cat(flat.tri_v1, v1), tri_e1=cat(flat.tri_e1, e1), tri_e2=cat(flat.tri_e2, e2),
                               tri_normal=cat(flat.tri_normal, nrm.astype(F32)), tri_material=cat(flat.tri_material, np.zeros(3, np.uint32))).contiguous()


def sphere_receiver_scene():
    """a sphere as the receiver (cube-map cells), panes beside, above and beyond it, lights on two sides"""
    quads = [([0.1, 0.1, 0.9], [0.8, 0, 0], [0, 0.8, 0]), ([0.9, 0.2, 0.2], [0, 0.6, 0], [0.05, 0, 0.6]), ([0.3, 0.3, 0.72], [0.1, 0, 0.01], [0, 0.1, 0])]
    return _soup(quads, spheres=[(0.5, 0.5, 0.5, 0.2)], lights=[[0.5, 0.5, 0.85, 1.0, 0.9, 0.8, 3.0], [0.95, 0.5, 0.5, 0.2, 0.3, 0.4, 1.5]])


# name -> (cfg, flat, every n-th cell)
CASES = {
    "synthetic": lambda: mc.workload("c3") + (None,),
    "far_side": lambda: (soft_cfg(), far_side_scene(), None),
    "sliver": lambda: (soft_cfg(), sliver_scene(), None),
    "sphere_receiver": lambda: (soft_cfg(), sphere_receiver_scene(), None),
    "semesterbild": lambda: (soft_cfg(), cases.flat_semesterbild(soft_cfg()), 1000),
}
MAX_CELLS = 48       # of a scene without a prescribed stride: evenly spread
MARGINAL_CAP = 400   # pruned triples per case the weak rule keeps
OTHERS = 100         # ... and of those it prunes too
RANDOM_POINTS = 16


class Case:
    pass


def load(probe, name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
    cfg, flat, stride = CASES[name]()
    k = Case()
    k.name, k.cfg, k.flat = name, cfg, flat
    k.desc, k.keep = _abi.make_scene_desc(flat)
    sizes = np.zeros(4, np.uint64)
    assert probe.probe_pack(C.byref(k.desc), C.c_uint64(budget), ptr(sizes)) == 0, probe.probe_error()
    k.blob, dev = np.zeros(int(sizes[0]), np.uint8), np.zeros(19, np.uint32)
    probe.probe_get(ptr(k.blob), ptr(dev))
    k.dev = {n: int(v) for n, v in zip(DEV_FIELDS, dev)}
    k.n_cells, k.n_tri_cells = int(sizes[2]), int(sizes[3])
    assert k.n_cells > 0, "the scene has receiver cells"
    cs = np.ascontiguousarray(sampling.cloud_sets(cfg), F32)
    f = np.array([cfg.fw, cfg.fh, cfg.fd], F32)
    scaled, out = np.zeros(cs.size // 3 * 4, F32), np.zeros(6, F32)
    probe.probe_consts(ptr(cs), C.c_uint64(cs.size), ptr(f), C.c_float(cfg.eps_distance), ptr(scaled), ptr(out))
    k.cloud = scaled.reshape(-1, 4)[:, :3].copy()
    k.centre, k.cloud_delta, k.beam_delta, k.eps_o = out[:3].copy(), out[3], out[4], out[5]
    ns = k.dev["n_slots"]
    o = k.dev["off_tri_isect"]
    k.isect = k.blob[o:o + 48 * ns].view(F32).reshape(ns, 12)
    o = k.dev["off_tri_id"]
    k.tri_id = k.blob[o:o + 4 * ns].view(np.uint32) & IDX
    k.lights = flat.lights.reshape(-1, 7)[:, :3].astype(F32)
    stride = stride or max(1, k.n_cells // MAX_CELLS)
    k.cells = list(range(stride // 2 if name != "semesterbild" else 0, k.n_cells, stride))
    return k


def pruned_of(probe, k, c, mode):
    out = np.zeros((k.dev["n_lights"], k.dev["n_slots"]), np.uint8)
    probe.probe_prune_all(c, mode, ptr(out))
    return out.astype(bool)


def hull_of(probe, c):
    out = np.zeros(27, F32)
    if not probe.probe_hull(c, ptr(out)):
        return None
    return out[:3].copy(), out[3:].reshape(8, 3).copy()


# ---- the rays and the literal test, float32 ------------------------------------------------------------------------------------------
def _dot_fused(a, b):
    """fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)) of rt_kernels.hip: the products are exact in float64"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    inner = (a[..., 2] * b[..., 2]).astype(F32).astype(np.float64)
    inner = (a[..., 1] * b[..., 1] + inner).astype(F32).astype(np.float64)
    return (a[..., 0] * b[..., 0] + inner).astype(F32)


def shadow_rays(h, lp, eps):
    """shadow_geom for every (hit point, light point): origins, unit directions (re-normalised as Ray::new does), tmax"""
    h, lp = np.broadcast_arrays(h[:, None, :], lp[None, :, :])
    h, lp = h.reshape(-1, 3).astype(F32), lp.reshape(-1, 3).astype(F32)
    ltp = (lp - h).astype(F32)
    ld = (ltp * (F32(1) / np.sqrt(_dot_fused(ltp, ltp)))[:, None]).astype(F32)
    so = (h + (ld * F32(eps)).astype(F32)).astype(F32)
    ls = (lp - so).astype(F32)
    tmax = np.sqrt(_dot_fused(ls, ls)).astype(F32)
    d = (ld * (F32(1) / np.sqrt(_dot_fused(ld, ld)))[:, None]).astype(F32)
    return so, d, tmax


def literal(q, o, d):
    """triangle_intersect of oracle/rt_oracle.c on float32 arrays, operation for operation -> (valid, t)"""
    v1, c1, c2 = q[0:3], -q[3:6], -q[6:9]
    b = (v1 - o).astype(F32)

    def cross(a, c):
        return np.stack([a[..., 1] * c[..., 2] + (-a[..., 2] * c[..., 1]), a[..., 2] * c[..., 0] + (-a[..., 0] * c[..., 2]),
                         a[..., 0] * c[..., 1] + (-a[..., 1] * c[..., 0])], -1).astype(F32)

    def dot(a, c):
        return ((a[..., 0] * c[..., 0] + a[..., 1] * c[..., 1]).astype(F32) + a[..., 2] * c[..., 2]).astype(F32)

    x, y, z = cross(c1, c2), cross(np.broadcast_to(c2, d.shape), d), cross(d, np.broadcast_to(c1, d.shape))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F32(1) / _dot_fused(d, np.broadcast_to(x, d.shape))).astype(F32)  # (vdot is the fused one)
        t = dot((x * inv[:, None]).astype(F32), b)
        u = dot((y * inv[:, None]).astype(F32), b)
        v = dot((z * inv[:, None]).astype(F32), b)
        det = ((d[:, 0] * (c1[1] * c2[2] - c2[1] * c1[2]) - c1[0] * (d[:, 1] * c2[2] - c2[1] * d[:, 2])).astype(F32) +
               c2[0] * (d[:, 1] * c1[2] - c1[1] * d[:, 2])).astype(F32)
        valid = ~(t <= EPS) & ~((u < 0) | (v < 0) | ((u + v).astype(F32) >= 1)) & ~(np.abs(det) <= EPS)
    return valid, t


def hit_points(rng, pm, pt):
    n1 = float(np.abs(pm).sum())
    # the surface normal at the centre: of the cell's plane (a triangle: pt[0..3] coplanar), or the direction of the hull's depth
    nrm = np.cross(pt[1] - pt[0], pt[2] - pt[0]).astype(np.float64)
    nrm /= max(np.linalg.norm(nrm), 1e-30)
    w = rng.dirichlet(np.ones(8), RANDOM_POINTS)
    pts = [pt, pm[None], (pm + 4e-7 * n1 * nrm)[None], (pm - 4e-7 * n1 * nrm)[None], w @ pt.astype(np.float64)]
    return np.concatenate(pts).astype(F32)


def light_points(k, l, pm, q):
    c = (k.lights[l] + k.centre).astype(F32)
    pts = [(k.lights[l][None] + k.cloud).astype(F32)]
    b, bc = q[0:3].astype(np.float64) - pm, q[0:3].astype(np.float64) - c
    c1, c2, x = -q[3:6].astype(np.float64), -q[6:9].astype(np.float64), q[9:12].astype(np.float64)
    for w in (np.cross(b, c2), np.cross(bc, c2), np.cross(c1, b), np.cross(c1, bc), x):
        n = np.linalg.norm(w)
        if n > 0:
            pts += [(c + float(k.beam_delta) * w / n)[None].astype(F32), (c - float(k.beam_delta) * w / n)[None].astype(F32)]
    return np.concatenate(pts)


def violations(probe, k, mode=FULL, seed=1):
    """-> (triples checked, rays cast, [(cell, light, slot, accepted rays)]) for the pruned triples of rule `mode`"""
    rng = np.random.default_rng(seed)
    cap = 1 << 20
    cells = np.asarray(k.cells, np.uint32)
    totals, nm, no = np.zeros(4, np.uint64), C.c_uint64(0), C.c_uint64(0)
    marginal, others = np.zeros((cap, 3), np.uint32), np.zeros((cap, 3), np.uint32)
    probe.probe_scan(ptr(cells), C.c_uint32(len(cells)), C.c_uint32(mode), ptr(totals), ptr(marginal), C.byref(nm), ptr(others), C.byref(no), C.c_uint64(cap),
                     C.c_uint32(max(1, len(cells) * k.dev["n_lights"] * k.dev["n_slots"] // 200000)))
    assert totals[3] == 0, "the weak rule prunes a subset of the full rule"
    assert nm.value <= cap and no.value <= cap
    # (the threads of the probe deliver in any order: sorted before the seeded choice)
    marginal, others = np.unique(marginal[:nm.value], axis=0), np.unique(others[:no.value], axis=0)
    take = lambda v, n: [tuple(int(x) for x in v[i]) for i in sorted(rng.choice(len(v), min(n, len(v)), replace=False))] if len(v) else []  # noqa: E731
    chosen = [p + (True,) for p in take(marginal, MARGINAL_CAP)] + [p + (False,) for p in take(others, OTHERS)]
    totals = totals.astype(np.int64)
    bad, rays = [], 0
    k.sample_rays = []
    for c, l, s, m in chosen:
        pm, pt = hull_of(probe, c)
        so, d, tmax = shadow_rays(hit_points(rng, pm, pt), light_points(k, l, pm.astype(np.float64), k.isect[s]), k.cfg.eps_distance)
        valid, t = literal(k.isect[s], so, d)
        acc = valid & (t <= tmax)
        rays += len(so)
        if acc.any():
            bad.append((c, l, s, int(acc.sum())))
        if len(k.sample_rays) < 64:
            i = int(rng.integers(len(so)))
            k.sample_rays.append((s, so[i].copy(), d[i].copy(), bool(valid[i]), float(t[i])))
    k.totals, k.n_marginal = totals, len(marginal)
    return len(chosen), rays, bad


@pytest.fixture(scope="module")
def loaded(probe):
    cache = {}

    def get(name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
        if (name, budget) not in cache:
            cache.clear()  # (the probe holds one packed scene)
            cache[name, budget] = load(probe, name, budget)
        return cache[name, budget]
    return get


# ---- tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_no_pruned_triangle_is_accepted_by_any_shadow_ray(probe, loaded, name):
    k = loaded(name)
    n, rays, bad = violations(probe, k)
    print(f"{name}: {len(k.cells)} cells, {k.totals[0]} triples, pruned {k.totals[1]} (weak rule {k.totals[2]}), marginal {k.n_marginal}, "
          f"checked {n} with {rays} rays, accepted {len(bad)}")
    assert n > 0 and k.totals[1] > 0, "the rule prunes something here"
    assert not bad, f"pruned but accepted (cell, light, slot, rays): {bad[:10]}"
    # the numpy restatement is the oracle's test: same verdict and same t on a sample of the rays just cast
    lib = oracle_lib.load()
    fp = C.POINTER(C.c_float)
    for s, o, d, valid, t in k.sample_rays:
        out = np.zeros(4, F32)
        got = lib.rt_oracle_triangle(C.byref(k.desc), int(k.tri_id[s]), o.ctypes.data_as(fp), d.ctypes.data_as(fp), 0, out.ctypes.data_as(fp))
        # (t to 4 ulp: the fused dot products are taken in float64 here and rounded twice)
        assert bool(got) == valid and (not got or abs(float(out[0]) - t) <= 5e-7 * abs(t)), (s, o, d, valid, t, got, out)


def test_the_far_side_rule_is_what_removes_the_pane_behind_the_light(probe, loaded):
    k = loaded("far_side")
    near, pane = np.nonzero((k.tri_id >= 2) & (k.tri_id < 4))[0], np.nonzero(k.tri_id >= 4)[0]
    with_far = without = 0
    for c in k.cells:
        if hull_of(probe, c) is None or c >= k.n_tri_cells:
            continue
        with_far += int(pruned_of(probe, k, c, FULL)[0, pane].sum())
        without += int(pruned_of(probe, k, c, EUCLID)[0, pane].sum())
    assert with_far > without, (with_far, without)


def test_lists_are_compacted_and_an_emptied_list_sets_the_clear_bit(probe, loaded):
    k = loaded("far_side", 48 * 6 + 8192)  # (a budget for at most 4096 cells: every one of them is looked at)
    nl, ns = k.dev["n_lights"], k.dev["n_slots"]
    rng = np.random.default_rng(3)
    lists = np.full((k.n_cells, nl, 8), END, np.uint16)
    for c in range(k.n_cells):
        for l in range(nl):
            n = min(int(rng.integers(0, 9)), ns)
            lists[c, l, :n] = rng.choice(ns, n, replace=False)
    lists[1::7, 0, 0] = OVERFLOW
    flags = rng.integers(0, 4, k.n_cells).astype(np.uint16) << 8  # (sphere bits: kept)
    before, fbefore = lists.copy(), flags.copy()
    probe.probe_prune_lists(FULL, ptr(lists), ptr(flags), k.n_cells)
    changed = 0
    for c in range(k.n_cells):
        active = hull_of(probe, c) is not None
        pruned = pruned_of(probe, k, c, FULL) if active else None
        want_flag = int(fbefore[c])
        for l in range(nl):
            row = before[c, l]
            if not active or row[0] >= OVERFLOW:
                assert np.array_equal(lists[c, l], row), "inactive, empty and overflowed lists are left alone"
                continue
            n = int(np.argmax(row >= OVERFLOW)) if (row >= OVERFLOW).any() else 8
            keep = [int(s) for s in row[:n] if not pruned[l, s]]
            assert list(lists[c, l]) == keep + [END] * (8 - len(keep)), (c, l)
            changed += len(keep) != n
            if not keep:
                want_flag |= 1 << l
        assert int(flags[c]) == want_flag, (c, int(flags[c]), want_flag)
    assert changed > 0
