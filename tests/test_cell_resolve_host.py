"""The stage that enumerates overflowed per-cell shadow candidate lists again (csrc/rt_cell_resolve.h) checked on the CPU,
through its host model (rt_resolve_walk / rt_cell_resolve_cell / rt_cell_resolve_packed, csrc/rt_cell_resolve.cpp -- the same
functions the kernel is made of), compiled host-only with the probe of test_cell_prune_host.py plus a few entry points.

Soundness, zero tolerance: the stage is offered EVERY leaf slot of the scene for every tested (cell, light) -- it walks the
whole tree -- and a slot it leaves out (not reached by the inflated segment, or rejected by the near-side rule or by
rt_prune_rule) must not be accepted by the literal triangle test for ANY shadow ray the render can cast from the cell towards
the light's cloud.  Of the triples left out the test takes every one that rt_prune_rule alone would keep (the ones only the
enumeration or the near-side rule removes: the marginal ones, up to a cap) and a seeded sample of the rest, and casts the rays
of test_cell_prune_host.py at them: hit points = the hull's 8 points, its centre, the centre pushed off the surface both ways,
random hull points; light points = every cloud point and the ball's extremes; the oracle's literal test in float32.

Ablations, run once each on semesterbild: the near-side bound taken at the cell's centre alone, and boxes without the
inflation by max(rho, delta); the triples only the ablated stage leaves out are checked, and each ablation must be caught.

Behaviour, on hand-built fans of panes (single triangles) over one receiver quad and one receiver sphere, with one light."""
import ctypes as C

import numpy as np
import pytest

import test_cell_prune_host as host
from test_cell_prune_host import END, F32, FULL, OVERFLOW, _soup, soft_cfg
from test_scene_pack_host import CSRC, HIPCC, ROOT, ptr
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

NEAR_CENTRE, NO_INFLATE, NO_NEAR = 0x100, 0x200, 0x400
BINS = ("0", "1-4", "5-8", "9-16", ">16")

PROBE = host.PROBE.replace('#include "rt_cell_prune.h"', '#include "rt_cell_resolve.h"') + r'''
static RtCellResolveArgs R;
extern "C" {
// after probe_consts: the stage's arguments for the same frame constants
void probe_resolve_consts(float eps) {
  RtDevParams P{};
  rt_beam_constants(eps, &P);
  R = RtCellResolveArgs();
  R.cell = A;
  R.eps_push = P.beam_eps_push, R.eps_ulp = P.beam_eps_ulp;
}
// the whole tree walked for every light of cell c: kept[l * n_slots + slot] = 1 for the survivors; returns 0 for a cell that is never looked up
static int resolve_all(uint32_t c, uint32_t mode, uint8_t* kept) {
  RtCellResolveArgs a = R;
  a.cell.mode = mode;
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  memset(kept, 0, (size_t)nl * ns);
  RtResolveCell K;
  if (!rt_resolve_cell_setup(g.dev, (const char*)g.blob.data(), a.cell, c, K)) return 0;
  for (uint32_t l = 0; l < nl; l++) {
    RtPruneBeam B;
    rt_resolve_beam(g.dev, (const char*)g.blob.data(), a.cell, K, l, B);
    if (!rt_resolve_walk(g.dev, (const char*)g.blob.data(), a, K, B, [&](uint32_t slot) { kept[(size_t)l * ns + slot] = 1; return true; })) return -1;
  }
  return 1;
}
int probe_resolve_all(uint32_t c, uint32_t mode, uint8_t* kept) { return resolve_all(c, mode, kept); }
// resolve_all over many cells on up to 16 threads.  base_resolve = 0: the base is rt_prune_rule(FULL) offered every slot
// (probe_prune_all); 1: the base is the stage itself with RT_PRUNE_FULL.  totals = {triples, left out by `mode`, left out by the
// base, left out by the base but kept by `mode`}; marginal = {cell, light, slot} left out by `mode` and kept by the base, others =
// every `every`-th (by a hash) of the rest of the left-out ones, both capped at `cap`; hist[5] = (cell, light) pairs by
// survivors under `mode`: 0, 1-4, 5-8, 9-16, more; hist[5] = their sum
void probe_resolve_scan(const uint32_t* cells, uint32_t n, uint32_t mode, uint32_t base_resolve, uint64_t* totals, uint32_t* marginal, uint64_t* n_marginal,
                        uint32_t* others, uint64_t* n_others, uint64_t cap, uint32_t every, uint64_t* hist) {
  const uint32_t nl = g.dev.n_lights, ns = g.dev.n_slots;
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::mutex mu;
  std::atomic<uint32_t> next{0};
  totals[0] = totals[1] = totals[2] = totals[3] = 0, *n_marginal = *n_others = 0;
  for (int k = 0; k < 6; k++) hist[k] = 0;
  auto work = [&]() {
    std::vector<uint8_t> km((size_t)nl * ns), kb((size_t)nl * ns);
    std::vector<uint32_t> mine, rest;
    uint64_t t[4] = {0, 0, 0, 0}, h[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i; (i = next++) < n;) {
      const uint32_t c = cells[i];
      if (resolve_all(c, mode, km.data()) != 1) continue;
      if (base_resolve) {
        resolve_all(c, RT_PRUNE_FULL, kb.data());
      } else {
        probe_prune_all(c, RT_PRUNE_FULL, kb.data());
        for (auto& x : kb) x = !x;
      }
      for (uint32_t l = 0; l < nl; l++) {
        uint32_t surv = 0;
        for (uint32_t s = 0; s < ns; s++) {
          const size_t k = (size_t)l * ns + s;
          surv += km[k];
          t[0]++, t[1] += !km[k], t[2] += !kb[k], t[3] += !kb[k] && km[k];
          if (!km[k] && kb[k]) mine.insert(mine.end(), {c, l, s});
          else if (!km[k] && (c * 2654435761u + l * 40503u + s * 97u) % every == 0u) rest.insert(rest.end(), {c, l, s});
        }
        h[surv == 0u ? 0 : surv <= 4u ? 1 : surv <= 8u ? 2 : surv <= 16u ? 3 : 4]++, h[5] += surv;
      }
    }
    std::lock_guard<std::mutex> lock(mu);
    for (int k = 0; k < 4; k++) totals[k] += t[k];
    for (int k = 0; k < 6; k++) hist[k] += h[k];
    for (size_t k = 0; k + 2 < mine.size(); k += 3, ++*n_marginal)
      if (*n_marginal < cap) memcpy(marginal + 3 * *n_marginal, &mine[k], 12);
    for (size_t k = 0; k + 2 < rest.size(); k += 3, ++*n_others)
      if (*n_others < cap) memcpy(others + 3 * *n_others, &rest[k], 12);
  };
  std::vector<std::thread> th;
  for (unsigned k = 0; k < nt; k++) th.emplace_back(work);
  for (auto& x : th) x.join();
}
// the host model on whole arrays ([n_cells][n_lights][8], [n_cells] and optionally [n_cells][n_lights] survivor counts), in place
void probe_resolve_lists(uint32_t mode, uint16_t* lists, uint16_t* flags, uint32_t n_cells, uint8_t* counts) {
  RtCellResolveArgs a = R;
  a.cell.mode = mode, a.cell.lists = lists, a.cell.flags = flags, a.cell.n_cells = n_cells, a.counts = counts;
  rt_cell_resolve_packed(g, a);
}
uint64_t rt_cell_resolve_temp_bytes_c(uint32_t n_cells, uint64_t left, uint32_t* chunk) { return rt_cell_resolve_temp_bytes(n_cells, (size_t)left, chunk); }
}
'''
SOURCES = ("rt_scene_pack.cpp", "rt_tables.cpp", "rt_bvh.cpp", "rt_cell_prune.cpp", "rt_cell_resolve.cpp")


def build_probe(d, text=PROBE):
    import os
    import subprocess
    src, so = d / "probe.cpp", d / "probe.so"
    src.write_text(text)
    out = subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                          "-shared", "-o", str(so), str(src)] + [os.path.join(CSRC, f) for f in SOURCES], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import os
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return build_probe(tmp_path_factory.mktemp("cell_resolve_probe"))


# ---- fans: panes (single triangles) over a receiver quad and a receiver sphere, one light ------------------------------------------
LIGHT = [0.5, 0.5, 0.6, 1.0, 0.9, 0.8, 3.0]
TILT = 2.0
FAN_BUDGET = 48 * 14 + 8192  # (as the GPU test packs them: at most 4096 receiver cells)


def _between(i):
    """the i-th level pane between the receivers and the light; the light's beam from the receiver quad and the sphere passes
    well inside every one of them.  Each is a little shorter than the one below it, so that on the panes themselves (they are
    receivers too) the number of panes a beam crosses changes from cell to cell"""
    return [-0.5, -0.5, 0.2 + 0.02 * i], [2.5 - 0.1 * i, 0.0, 0.0], [0.0, 2.5, 0.0]


def _behind(dz):
    """a tilted pane that passes dz above the light: behind it for every ray from below, yet its box reaches down over the
    light, so a box test along the beam keeps it"""
    return [-0.3, -0.3, LIGHT[2] + dz - 0.8 * TILT], [2.0, 0.0, 2.0 * TILT], [0.0, 2.0, 0.0]


def fan_scene(n_between, n_behind):
    panes = [_between(i) for i in range(n_between)] + [_behind(0.8 + 0.02 * i) for i in range(n_behind)]
    flat = _soup([([0.3, 0.3, 0], [0.4, 0, 0], [0, 0.4, 0])], spheres=[(0.5, 0.5, 0.06, 0.05)], lights=[LIGHT])
    v1, e1, e2 = (np.array([p[i] for p in panes], F32) for i in range(3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    import dataclasses
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])  # noqa: E731
    return dataclasses.replace(flat, tri_v1=cat(flat.tri_v1, v1), tri_e1=cat(flat.tri_e1, e1), tri_e2=cat(flat.tri_e2, e2), tri_normal=cat(flat.tri_normal, nrm.astype(F32)),
                               tri_material=cat(flat.tri_material, np.zeros(len(panes), np.uint32))).contiguous()


# name -> (panes between, panes behind the light)
FANS = {"fan_behind": (0, 12), "fan_mixed": (3, 9), "fan_between": (12, 0)}
for _name, (_a, _b) in FANS.items():
    host.CASES[_name] = (lambda a=_a, b=_b: (soft_cfg(), fan_scene(a, b), None))
SOUND_CASES = ["synthetic", "far_side", "sliver", "sphere_receiver", "semesterbild"] + list(FANS)


def load(probe, name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
    k = host.load(probe, name, budget)
    probe.probe_resolve_consts(C.c_float(k.cfg.eps_distance))
    return k


@pytest.fixture(scope="module")
def loaded(probe):
    cache = {}

    def get(name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
        if (name, budget) not in cache:
            cache.clear()  # (the probe holds one packed scene)
            cache[name, budget] = load(probe, name, budget)
        return cache[name, budget]
    return get


def kept_of(probe, k, c, mode=FULL):
    out = np.zeros((k.dev["n_lights"], k.dev["n_slots"]), np.uint8)
    rc = probe.probe_resolve_all(c, mode, ptr(out))
    assert rc >= 0, "the walk found the tree broken"
    return out.astype(bool) if rc else None


def violations(probe, k, mode=FULL, base_resolve=0, seed=1, marginal_cap=host.MARGINAL_CAP, others_n=host.OTHERS):
    """-> (triples checked, rays cast, [(cell, light, slot, accepted rays)]) for the triples the stage leaves out under `mode`"""
    rng = np.random.default_rng(seed)
    cap = 1 << 20
    cells = np.asarray(k.cells, np.uint32)
    totals, hist, nm, no = np.zeros(4, np.uint64), np.zeros(6, np.uint64), C.c_uint64(0), C.c_uint64(0)
    marginal, others = np.zeros((cap, 3), np.uint32), np.zeros((cap, 3), np.uint32)
    probe.probe_resolve_scan(ptr(cells), C.c_uint32(len(cells)), C.c_uint32(mode), C.c_uint32(base_resolve), ptr(totals), ptr(marginal), C.byref(nm), ptr(others),
                             C.byref(no), C.c_uint64(cap), C.c_uint32(max(1, len(cells) * k.dev["n_lights"] * k.dev["n_slots"] // 200000)), ptr(hist))
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
        if acc.any():
            bad.append((c, l, s, int(acc.sum())))
    k.totals, k.hist, k.n_marginal = totals.astype(np.int64), hist.astype(np.int64), len(marginal)
    return len(chosen), rays, bad


# ---- soundness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOUND_CASES)
def test_no_slot_the_stage_leaves_out_is_accepted_by_any_shadow_ray(probe, loaded, name):
    k = loaded(name, FAN_BUDGET if name in FANS else _abi.RT_SCENE_BUDGET_DEFAULT)
    n, rays, bad = violations(probe, k)
    pairs = int(k.hist[:5].sum())
    print(f"{name}: {len(k.cells)} cells, {k.totals[0]} triples, left out {k.totals[1]} (rt_prune_rule alone {k.totals[2]}), marginal {k.n_marginal}, "
          f"checked {n} with {rays} rays, accepted {len(bad)}; survivors per (cell, light) "
          f"{dict(zip(BINS, (int(v) for v in k.hist[:5])))}, mean {k.hist[5] / max(1, pairs):.2f}")
    assert n > 0 and k.totals[1] > 0, "the stage leaves something out here"
    assert k.totals[3] == 0, "what rt_prune_rule removes, the stage removes"
    assert not bad, f"left out but accepted (cell, light, slot, rays): {bad[:10]}"


# ---- ablations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, mode", [("near side at the centre only", FULL | NEAR_CENTRE), ("no box inflation", FULL | NO_INFLATE)])
def test_an_unsound_variant_is_caught(probe, loaded, what, mode):
    k = loaded("semesterbild")
    n, rays, bad = violations(probe, k, mode=mode, base_resolve=1, marginal_cap=3000, others_n=0)
    print(f"{what}: {k.n_marginal} triples left out beyond the stage's own, checked {n} with {rays} rays, accepted by some ray: {len(bad)} triples, "
          f"{sum(b[3] for b in bad)} rays")
    assert k.n_marginal > 0, "the ablation removes more"
    assert bad, f"{what}: not caught at these sizes"


def test_the_near_side_rule_is_what_brings_the_lists_under_eight(probe, loaded):
    """profiles/r08_cell_prune.md, step 1: rt_prune_rule alone keeps "the surface the point lies on and everything behind it\""""
    k = loaded("semesterbild")
    violations(probe, k, mode=FULL | NO_NEAR, marginal_cap=0, others_n=0)
    without = k.hist.copy()
    violations(probe, k, mode=FULL, marginal_cap=0, others_n=0)
    print(f"survivors per (cell, light), all slots offered: without the near side {dict(zip(BINS, map(int, without[:5])))} sum {without[5]}, "
          f"with it {dict(zip(BINS, map(int, k.hist[:5])))} sum {k.hist[5]}")
    assert k.hist[5] < without[5] and k.hist[3] + k.hist[4] < without[3] + without[4]


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
def resolve_everything(probe, k):
    """every list of the scene set to the overflow marker and resolved by the host model -> lists, flags, survivor counts"""
    nl = k.dev["n_lights"]
    lists = np.full((k.n_cells, nl, 8), END, np.uint16)
    lists[:, :, 0] = OVERFLOW
    flags, counts = np.zeros(k.n_cells, np.uint16), np.zeros((k.n_cells, nl), np.uint8)
    probe.probe_resolve_lists(FULL, ptr(lists), ptr(flags), k.n_cells, ptr(counts))
    return lists, flags, counts


def fan_slots(k, n_between):
    """leaf slots of the panes between the receivers and the light, and of those behind it (canonical triangles 0, 1: the quad)"""
    return set(np.nonzero((k.tri_id >= 2) & (k.tri_id < 2 + n_between))[0].tolist()), set(np.nonzero(k.tri_id >= 2 + n_between)[0].tolist())


def centre_cells(probe, k):
    """the quad's cells around (0.5, 0.5, 0) and the sphere's cells around its top"""
    quad, sphere = [], []
    for c in range(k.n_cells):
        h = host.hull_of(probe, c)
        if h is None:
            continue
        pm = h[0]
        if c < k.n_tri_cells and abs(pm[2]) < 1e-6 and abs(pm[0] - 0.5) < 0.1 and abs(pm[1] - 0.5) < 0.1:
            quad.append(c)
        if c >= k.n_tri_cells and pm[2] > 0.06 + 0.045:
            sphere.append(c)
    assert quad and sphere
    return quad, sphere


@pytest.mark.parametrize("name", list(FANS))
def test_fans(probe, loaded, name):
    k = loaded(name, FAN_BUDGET)
    n_between, n_behind = FANS[name]
    between, behind = fan_slots(k, n_between)
    assert len(between) == n_between and len(behind) == n_behind and k.dev["n_slots"] == 14, "one leaf slot per triangle"
    lists, flags, counts = resolve_everything(probe, k)
    quad, sphere = centre_cells(probe, k)
    for kind, cells in (("quad", quad), ("sphere", sphere)):
        for c in cells:
            got = [int(s) for s in lists[c, 0] if s < OVERFLOW]
            if name == "fan_behind":
                assert list(lists[c, 0]) == [END] * 8 and counts[c, 0] == 0 and flags[c] & 1, (kind, c, lists[c, 0], counts[c, 0])
            elif name == "fan_mixed":
                assert set(got) == between and len(got) == 3 and lists[c, 0, 3] == END and counts[c, 0] == 3 and not flags[c] & 1, (kind, c, lists[c, 0])
            else:
                assert lists[c, 0, 0] == OVERFLOW and counts[c, 0] == 12 and not flags[c] & 1, (kind, c, lists[c, 0], counts[c, 0])
    # without the survivor counts the walk ends at the ninth survivor: same words
    lists2 = np.full_like(lists, END)
    lists2[:, :, 0] = OVERFLOW
    flags2 = np.zeros_like(flags)
    probe.probe_resolve_lists(FULL, ptr(lists2), ptr(flags2), k.n_cells, None)
    assert np.array_equal(lists, lists2) and np.array_equal(flags, flags2)


def test_a_list_that_is_not_overflowed_is_not_touched(probe, loaded):
    k = loaded("fan_mixed", FAN_BUDGET)
    nl, ns = k.dev["n_lights"], k.dev["n_slots"]
    rng = np.random.default_rng(5)
    lists = np.full((k.n_cells, nl, 8), END, np.uint16)
    for c in range(k.n_cells):
        n = int(rng.integers(0, 9))
        lists[c, 0, :n] = rng.choice(ns, n, replace=False)
    lists[1::3, 0, :] = END
    lists[1::3, 0, 0] = OVERFLOW
    flags = (rng.integers(0, 4, k.n_cells).astype(np.uint16) << 8) | (rng.integers(0, 2, k.n_cells).astype(np.uint16) << 1)  # (other bits: kept)
    before, fbefore = lists.copy(), flags.copy()
    probe.probe_resolve_lists(FULL, ptr(lists), ptr(flags), k.n_cells, None)
    over = before[:, 0, 0] == OVERFLOW
    assert np.array_equal(lists[~over], before[~over]) and np.array_equal(flags[~over], fbefore[~over]), "word for word"
    changed = resolved = 0
    for c in np.nonzero(over)[0]:
        kept = kept_of(probe, k, int(c))
        if kept is None:
            assert np.array_equal(lists[c], before[c]) and flags[c] == fbefore[c], "a cell that is never looked up is left alone"
            continue
        want = np.nonzero(kept[0])[0]
        if len(want) > 8:
            assert np.array_equal(lists[c], before[c]) and flags[c] == fbefore[c]
            continue
        resolved += 1
        assert sorted(int(s) for s in lists[c, 0] if s < OVERFLOW) == sorted(want.tolist()) and list(lists[c, 0, len(want):]) == [END] * (8 - len(want)), c
        assert int(flags[c]) == int(fbefore[c]) | (1 if len(want) == 0 else 0), c
        changed += 1
    assert resolved > 0 and changed > 0


def test_the_work_list_fits_its_bound(probe):
    """rt_cell_resolve_temp_bytes: never more than 64 MiB, never more than the budget leaves, at most 1024 chunks"""
    probe.rt_cell_resolve_temp_bytes_c.restype = C.c_uint64
    for n_cells, left in [(1, 1 << 30), (4096, 8192), (10_607_170, 1 << 30), (100_000_000, 1 << 30), (3_000_000_000, 1 << 30), (1000, 100), (1 << 20, 6000)]:
        chunk = C.c_uint32(0)
        b = probe.rt_cell_resolve_temp_bytes_c(C.c_uint32(n_cells), C.c_uint64(left), C.byref(chunk))
        assert b <= min(left, 64 << 20)
        if b:
            assert b == 4096 + 4 * chunk.value and 0 < chunk.value <= n_cells and -(-n_cells // chunk.value) <= 1024
        else:
            assert chunk.value == 0
    chunk = C.c_uint32(0)
    assert probe.rt_cell_resolve_temp_bytes_c(C.c_uint32(10_607_170), C.c_uint64(1 << 30), C.byref(chunk)) == 4096 + 4 * 10_607_170
