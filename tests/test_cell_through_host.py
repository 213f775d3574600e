"""The rule that marks the listed glass panes every shadow ray of a receiver cell crosses (csrc/rt_cell_through.h) checked on the
CPU, through its host model (rt_through_rule / rt_cell_through_cell / rt_cell_through_packed, csrc/rt_cell_through.cpp -- the same
functions the kernel is made of), compiled host-only with the probe of test_cell_resolve_host.py plus a few entry points.

Soundness, zero tolerance: a marked (cell, light, triangle) must be ACCEPTED by the literal triangle test, with t <= tmax, for
EVERY shadow ray the render can cast from the cell towards the light's cloud.  The probe offers every leaf slot of the scene to
the rule for every tested (cell, light), transmissive or not, which is more than a list would ever hold.  Of the marked triples
the test takes every one that a beam half again as fat (rho and delta times 1.5) would not mark -- the marginal ones, up to a
cap -- and a seeded sample of the rest, and casts the rays of test_cell_prune_host.py at them: hit points = the hull's 8 points,
its centre, the centre pushed off the surface both ways, random hull points; light points = every cloud point of every set and
the ball's extremes along +-w, +-w_c, +-X; the oracle's literal test in float32.

Known answers on a floor under one light with panes at half height, by the host model on hand-written lists; two ablations
(the rule without rho |w_c|, the rule without the near side), each of which must be caught; and the share of marked entries
on the semesterbild sample, whose lists are what the resolve stage's walk keeps for the cell."""
import ctypes as C

import numpy as np
import pytest

import test_cell_prune_host as host
import test_cell_resolve_host as rh
from test_cell_prune_host import END, F32, OVERFLOW, _quad, soft_cfg
from test_scene_pack_host import MAT_DIFFUSE, MAT_GLASS, flat_of, ptr
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

NO_RHO_WC, NO_NEAR = 1, 2
TRANSMISSIVE = 0x40000000

PROBE = rh.PROBE.replace('#include "rt_cell_resolve.h"', '#include "rt_cell_through.h"') + r'''
extern "C" {
// every leaf slot offered to the rule for every light of cell c: marked[l * n_slots + slot]; fat != 0: on a beam whose rho and
// delta are 1.5 times as large.  Returns 0 for a cell that is never looked up
static int through_all(uint32_t c, uint32_t mode, int fat, uint8_t* marked) {
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  const char* base = (const char*)g.blob.data();
  memset(marked, 0, (size_t)nl * ns);
  RtResolveCell K;
  if (!rt_resolve_cell_setup(g.dev, base, A, c, K)) return 0;
  const float* isect = (const float*)(base + g.dev.off_tri_isect);
  for (uint32_t l = 0; l < nl; l++) {
    RtPruneBeam B;
    rt_resolve_beam(g.dev, base, A, K, l, B);
    if (fat) B.lenp += 0.5f * (B.rho + B.delta), B.rho *= 1.5f, B.delta *= 1.5f;
    for (uint32_t s = 0; s < ns; s++) marked[(size_t)l * ns + s] = rt_through_rule(B, isect + 12u * (size_t)s, mode) ? 1 : 0;
  }
  return 1;
}
int probe_through_all(uint32_t c, uint32_t mode, uint8_t* marked) { return through_all(c, mode, 0, marked); }
// through_all over many cells on up to 16 threads.  totals = {triples, marked by `mode`, marked by the shipped rule (mode 0), marked
// by the shipped rule but not by `mode`}.  mode == 0: marginal = the {cell, light, slot} marked on the beam but not on the fat one,
// others = every `every`-th (by a hash) of the rest of the marked ones.  mode != 0 (an ablation): marginal = marked by `mode` and
// not by the shipped rule, others stays empty.  Both capped at `cap`
void probe_through_scan(const uint32_t* cells, uint32_t n, uint32_t mode, uint64_t* totals, uint32_t* marginal, uint64_t* n_marginal, uint32_t* others,
                        uint64_t* n_others, uint64_t cap, uint32_t every) {
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::mutex mu;
  std::atomic<uint32_t> next{0};
  totals[0] = totals[1] = totals[2] = totals[3] = 0, *n_marginal = *n_others = 0;
  auto work = [&]() {
    std::vector<uint8_t> mm((size_t)nl * ns), mb((size_t)nl * ns);
    std::vector<uint32_t> mine, rest;
    uint64_t t[4] = {0, 0, 0, 0};
    for (uint32_t i; (i = next++) < n;) {
      const uint32_t c = cells[i];
      if (through_all(c, mode, 0, mm.data()) != 1) continue;
      through_all(c, 0u, mode == 0u ? 1 : 0, mb.data());  // the fat beam, or the shipped rule
      for (uint32_t l = 0; l < nl; l++)
        for (uint32_t s = 0; s < ns; s++) {
          const size_t k = (size_t)l * ns + s;
          t[0]++, t[1] += mm[k], t[2] += mode == 0u ? mm[k] : mb[k], t[3] += mode != 0u && mb[k] && !mm[k];
          if (mm[k] && !mb[k]) mine.insert(mine.end(), {c, l, s});
          else if (mode == 0u && mm[k] && (c * 2654435761u + l * 40503u + s * 97u) % every == 0u) rest.insert(rest.end(), {c, l, s});
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
// the host model on whole arrays: lists [n_cells][n_lights][8], marks [n_cells * n_lights] bytes, written backwards from their end
void probe_through_lists(uint32_t mode, uint16_t* lists, uint32_t n_cells, uint8_t* marks) {
  RtCellThroughArgs a{};
  a.cell = A;
  a.cell.lists = lists, a.cell.n_cells = n_cells;
  a.marks_end = marks + (size_t)n_cells * g.dev.n_lights;
  a.mode = mode;
  rt_cell_through_packed(g, a);
}
// the lists the resolve stage's walk gives the sampled cells (at most 8 survivors: a list; else none), and their marks.
// stats[l * 4 ..] = {lists with an entry, listed transmissive entries, marked entries, lists with a transmissive entry whose every
// transmissive entry is marked}
void probe_through_sample(const uint32_t* cells, uint32_t n, uint64_t* stats) {
  const uint32_t nl = g.dev.n_lights;
  const char* base = (const char*)g.blob.data();
  const uint32_t* tri_id = (const uint32_t*)(base + g.dev.off_tri_id);
  std::vector<uint8_t> marks((size_t)g.n_cells * nl);
  RtCellThroughArgs a{};
  a.cell = A;
  a.marks_end = marks.data() + marks.size();
  for (uint32_t l = 0; l < nl * 4u; l++) stats[l] = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = cells[i];
    RtResolveCell K;
    if (!rt_resolve_cell_setup(g.dev, base, A, c, K)) continue;
    alignas(16) uint16_t list[8 * RT_PRUNE_LIST_SLOTS];
    for (auto& x : list) x = (uint16_t)RT_PRUNE_LIST_END;
    for (uint32_t l = 0; l < nl; l++) {
      RtPruneBeam B;
      rt_resolve_beam(g.dev, base, A, K, l, B);
      uint32_t cnt = 0;
      uint16_t* w = list + l * RT_PRUNE_LIST_SLOTS;
      const bool ok = rt_resolve_walk(g.dev, base, R, K, B, [&](uint32_t slot) { if (cnt < RT_PRUNE_LIST_SLOTS) w[cnt] = (uint16_t)slot; cnt++; return cnt <= RT_PRUNE_LIST_SLOTS; });
      if (!ok || cnt > RT_PRUNE_LIST_SLOTS) w[0] = (uint16_t)RT_PRUNE_LIST_OVERFLOW;
    }
    rt_cell_through_cell(g.dev, base, a, c, list);
    for (uint32_t l = 0; l < nl; l++) {
      const uint16_t* w = list + l * RT_PRUNE_LIST_SLOTS;
      if (w[0] >= RT_PRUNE_LIST_OVERFLOW) continue;
      const uint32_t m = a.marks_end[-1 - (ptrdiff_t)((size_t)c * nl + l)];
      uint32_t nt = 0, nm = 0;
      for (uint32_t k = 0; k < RT_PRUNE_LIST_SLOTS && w[k] < RT_PRUNE_LIST_OVERFLOW; k++)
        if (tri_id[w[k]] & RT_TRI_TRANSMISSIVE) nt++, nm += (m >> k) & 1u;
      stats[l * 4u] += 1, stats[l * 4u + 1u] += nt, stats[l * 4u + 2u] += nm, stats[l * 4u + 3u] += nt != 0u && nm == nt;
    }
  }
}
}
'''
SOURCES = rh.SOURCES + ("rt_cell_through.cpp",)


def build_probe(d):
    import os
    import subprocess
    from test_scene_pack_host import CSRC, HIPCC, ROOT
    src, so = d / "probe.cpp", d / "probe.so"
    src.write_text(PROBE)
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                          "-shared", "-o", str(so), str(src)] + [os.path.join(CSRC, f) for f in SOURCES], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import os
    if not os.path.exists(rh.HIPCC):
        pytest.skip("no hipcc")
    return build_probe(tmp_path_factory.mktemp("cell_through_probe"))


# ---- the pane scene: a floor under one light, panes at half height ------------------------------------------------------------------
# A shadow ray from the floor point (x, y, 0) to the light (0.5, 0.5, 0.6) crosses the plane z = 0.3 at ((x + 0.5) / 2, (y + 0.5) / 2).
LIGHT = [0.5, 0.5, 0.6, 1.0, 0.9, 0.8, 3.0]
Z = 0.3
# canonical triangle -> what it is.  0, 1: the floor
ACROSS, EDGE, DIAG_A, DIAG_B, BEHIND, OPAQUE = 2, 3, 4, 5, 6, 7


def pane_scene(second_light=False):
    tri = lambda v, a, b: ([np.asarray(v, np.float64)], [np.asarray(a, np.float64)], [np.asarray(b, np.float64)])  # noqa: E731
    parts = [_quad([0, 0, 0], [1, 0, 0], [0, 1, 0]),               # the floor
             tri([-1, -1, Z], [4, 0, 0], [0, 4, 0]),                # ACROSS: x + y < 2 at z = 0.3, every beam passes well inside
             tri([0.5, -1, Z + 0.01], [4, 0, 0], [0, 4, 0]),        # EDGE: its edge x = 0.5 runs through the beams of the floor's middle
             _quad([-1, -1.2, Z + 0.02], [3, 0, 0], [0, 3, 0]),     # DIAG_A, DIAG_B: the shared diagonal x + y = 0.8 cuts the beams
             tri([-1, -1, 0.9], [4, 0, 0], [0, 4, 0]),              # BEHIND: above the light
             tri([-1, -1, Z + 0.03], [4, 0, 0], [0, 4, 0])]         # OPAQUE: as ACROSS, diffuse
    v1, e1, e2 = (sum((p[i] for p in parts), []) for i in range(3))
    nrm = np.cross(np.asarray(e1), np.asarray(e2))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tm = [0, 0, 1, 1, 1, 1, 1, 0]
    lights = [LIGHT] + ([[0.2, 0.8, 0.5, 0.2, 0.3, 0.4, 1.5]] if second_light else [])
    return flat_of(v1=v1, e1=e1, e2=e2, nrm=nrm, tm=tm, mats=[MAT_DIFFUSE, MAT_GLASS], lights=lights).contiguous()


PANE_BUDGET = 1000000  # (receiver cells of about 0.011: some 8000 on the floor)
host.CASES["panes"] = lambda: (soft_cfg(), pane_scene(), None)
host.CASES["panes_two_lights"] = lambda: (soft_cfg(), pane_scene(True), None)
SOUND_CASES = ["synthetic", "far_side", "sliver", "sphere_receiver", "semesterbild", "panes"]


@pytest.fixture(scope="module")
def loaded(probe):
    cache = {}

    def get(name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
        if (name, budget) not in cache:
            cache.clear()  # (the probe holds one packed scene)
            cache[name, budget] = rh.load(probe, name, budget)
            k = cache[name, budget]
            o = k.dev["off_tri_id"]
            k.transmissive = (k.blob[o:o + 4 * k.dev["n_slots"]].view(np.uint32) & TRANSMISSIVE) != 0
        return cache[name, budget]
    return get


def marked_of(probe, k, c, mode=0):
    out = np.zeros((k.dev["n_lights"], k.dev["n_slots"]), np.uint8)
    return out.astype(bool) if probe.probe_through_all(c, mode, ptr(out)) else None


def marks_of(probe, k, lists, mode=0):
    """the host model on whole lists -> marks[cell, light] (the table is written backwards from its end)"""
    n_cells, nl = lists.shape[:2]
    raw = np.full(n_cells * nl, 0xAB, np.uint8)
    probe.probe_through_lists(mode, ptr(lists), n_cells, ptr(raw))
    return raw[::-1].reshape(n_cells, nl).copy()


def rejected(probe, k, mode=0, seed=1, marginal_cap=400, others_n=200):
    """-> (triples checked, rays cast, [(cell, light, slot, rejected rays)]) for the triples marked under `mode`"""
    rng = np.random.default_rng(seed)
    cap = 1 << 20
    cells = np.asarray(k.cells, np.uint32)
    totals, nm, no = np.zeros(4, np.uint64), C.c_uint64(0), C.c_uint64(0)
    marginal, others = np.zeros((cap, 3), np.uint32), np.zeros((cap, 3), np.uint32)
    probe.probe_through_scan(ptr(cells), C.c_uint32(len(cells)), C.c_uint32(mode), ptr(totals), ptr(marginal), C.byref(nm), ptr(others), C.byref(no), C.c_uint64(cap),
                             C.c_uint32(max(1, len(cells) * k.dev["n_lights"] * k.dev["n_slots"] // 200000)))
    nm, no = min(nm.value, cap), min(no.value, cap)
    marginal, others = np.unique(marginal[:nm], axis=0), np.unique(others[:no], axis=0)
    take = lambda v, n: [tuple(int(x) for x in v[i]) for i in sorted(rng.choice(len(v), min(n, len(v)), replace=False))] if len(v) else []  # noqa: E731
    chosen = take(marginal, marginal_cap) + take(others, others_n)
    bad, rays = [], 0
    for c, l, s in chosen:
        pm, pt = host.hull_of(probe, c)
        so, d, tmax = host.shadow_rays(host.hit_points(rng, pm, pt), host.light_points(k, l, pm.astype(np.float64), k.isect[s]), k.cfg.eps_distance)
        valid, t = host.literal(k.isect[s], so, d)
        acc = valid & (t <= tmax)
        rays += len(so)
        if not acc.all():
            bad.append((c, l, s, int((~acc).sum())))
    k.totals, k.n_marginal = totals.astype(np.int64), len(marginal)
    return len(chosen), rays, bad


# ---- soundness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOUND_CASES)
def test_every_shadow_ray_is_accepted_by_a_marked_triangle(probe, loaded, name):
    k = loaded(name, PANE_BUDGET if name == "panes" else _abi.RT_SCENE_BUDGET_DEFAULT)
    n, rays, bad = rejected(probe, k)
    print(f"{name}: {len(k.cells)} cells, {k.totals[0]} triples, marked {k.totals[1]}, marginal (not marked on a beam 1.5 times as fat) {k.n_marginal}, "
          f"checked {n} with {rays} rays, rejected {len(bad)}")
    if name in ("semesterbild", "panes"):
        assert n > 0 and k.totals[1] > 0, "the rule marks something here"
    assert not bad, f"marked but rejected (cell, light, slot, rays): {bad[:10]}"


# ---- ablations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, mode", [("without rho |w_c|", NO_RHO_WC), ("without the near side", NO_NEAR)])
def test_an_unsound_variant_is_caught(probe, loaded, what, mode):
    k = loaded("semesterbild")
    n, rays, bad = rejected(probe, k, mode=mode, marginal_cap=3000, others_n=0)
    print(f"{what}: {k.n_marginal} triples marked beyond the rule's own, checked {n} with {rays} rays, rejected by some ray: {len(bad)} triples, "
          f"{sum(b[3] for b in bad)} rays")
    assert k.totals[3] == 0, "what the rule marks, the ablated rule marks"
    assert k.n_marginal > 0, "the ablation marks more"
    assert bad, f"{what}: not caught at these sizes"


# ---- known answers -------------------------------------------------------------------------------------------------------------
def _floor_cells(probe, k):
    """[(cell, centre, hull points)] of the floor's cells that are looked up (the floor's two triangles come first), and the
    first 40 cells of the ACROSS pane, which follows them"""
    floor, own = [], []
    for c in range(k.n_tri_cells):
        h = host.hull_of(probe, c)
        if h is None:
            continue
        if abs(float(h[0][2])) < 1e-6:
            floor.append((c, h[0].astype(np.float64), h[1].astype(np.float64)))
        elif abs(float(h[0][2]) - Z) < 1e-6:
            own.append(c)
            if len(own) == 40:
                break
        else:
            break
    return floor, own


def _slot_of(k, tri):
    s = np.nonzero(k.tri_id == tri)[0]
    assert len(s) == 1
    return int(s[0])


def test_known_answers_on_the_panes(probe, loaded):
    k = loaded("panes", PANE_BUDGET)
    nl = k.dev["n_lights"]
    floor, own = _floor_cells(probe, k)
    assert len(floor) > 2000 and own
    slot = {t: _slot_of(k, t) for t in (ACROSS, EDGE, DIAG_A, DIAG_B, BEHIND, OPAQUE)}
    assert k.transmissive[slot[ACROSS]] and not k.transmissive[slot[OPAQUE]]
    order = [ACROSS, EDGE, DIAG_A, DIAG_B, BEHIND, OPAQUE]
    lists = np.full((k.n_cells, nl, 8), END, np.uint16)
    for c, _, _ in floor:
        lists[c, 0, :6] = [slot[t] for t in order]
    # cells of the ACROSS pane itself (a receiver too) that list their own pane; one floor cell with an overflowed list
    for c in own:
        lists[c, 0, 0] = slot[ACROSS]
    over = floor[0][0]
    lists[over, 0, 0] = OVERFLOW
    before = lists.copy()
    marks = marks_of(probe, k, lists)
    assert np.array_equal(lists, before), "the stage only reads the lists"
    bit = {t: 1 << i for i, t in enumerate(order)}
    half = cut = right = 0
    for c, pm, pt in floor:
        m = int(marks[c, 0])
        if c == over:
            assert m == 0, "an overflowed list gets no marks"
            continue
        assert m & bit[ACROSS], f"cell {c}: a pane across the whole beam is marked"
        assert not m & bit[BEHIND], "a pane behind the light is not marked"
        assert not m & bit[OPAQUE], "an opaque pane is not marked"
        assert not m & ~0x3F
        # where the segments from the cell's hull points to the light cross the planes of the EDGE pane and of the quad
        cross = lambda z: pt[:, :2] + (z / LIGHT[2]) * (np.asarray(LIGHT[:2]) - pt[:, :2])  # noqa: E731
        xs, ss = cross(Z + 0.01)[:, 0], cross(Z + 0.02).sum(1)
        if xs.min() < 0.5 < xs.max():  # the edge x = 0.5 runs through this cell's beam
            assert not m & bit[EDGE], f"cell {c}: a pane whose edge cuts the beam is not marked"
            cut += 1
        if xs.min() > 0.62:  # (the rule's slack at these coarse cells is about 0.1 on the pane)
            assert m & bit[EDGE]
            right += 1
        if xs.max() < 0.48:
            assert not m & bit[EDGE]
        if ss.min() < 0.8 < ss.max():  # the quad's diagonal x + y = 0.8 runs through the beam
            assert not m & (bit[DIAG_A] | bit[DIAG_B]), f"cell {c}: neither half of a quad whose diagonal cuts the beam is marked"
            half += 1
        if ss.min() > 0.95 or ss.max() < 0.65:
            assert bool(m & bit[DIAG_A]) != bool(m & bit[DIAG_B]), f"cell {c}: away from the diagonal exactly one half is marked"
    assert cut and right and half, (cut, right, half)
    for c in own:
        assert marks[c, 0] == 0, "a receiver cell lying on the pane itself is not marked"
    other = np.ones(k.n_cells, bool)
    other[[c for c, _, _ in floor] + own] = False
    assert not marks[other].any() and not marks[:, 1:].any(), "an empty list gets no marks"
    # the rule itself says the same of the opaque pane as of the glass one: the transmissive flag is what keeps it unmarked
    mk = marked_of(probe, k, floor[len(floor) // 2][0])
    assert mk[0, slot[ACROSS]] and mk[0, slot[OPAQUE]] and not mk[0, slot[BEHIND]]


# ---- the semesterbild sample -----------------------------------------------------------------------------------------------------
def test_most_listed_panes_of_the_light_under_the_glass_floor_are_marked(probe, loaded):
    """Marked share of listed transmissive entries per light (every 1000th cell; copied into profiles/r11_cell_through.md).  Only a
    floor against a rule that marks nothing is asserted: light 3 stands under the glass floor slab."""
    k = loaded("semesterbild")
    nl = k.dev["n_lights"]
    cells = np.asarray(k.cells, np.uint32)
    stats = np.zeros(nl * 4, np.uint64)
    probe.probe_through_sample(ptr(cells), C.c_uint32(len(cells)), ptr(stats))
    stats = stats.reshape(nl, 4).astype(np.int64)
    for l in range(nl):
        lists, listed, marked, full = (int(v) for v in stats[l])
        print(f"light {l}: {lists} lists, {listed} listed transmissive entries, {marked} marked ({100.0 * marked / max(1, listed):.1f} %), "
              f"{full} lists whose every transmissive entry is marked")
    assert stats[3, 1] > 100 and stats[3, 2] > 0.5 * stats[3, 1], stats[3]
