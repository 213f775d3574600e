"""Wide records of the per-cell shadow candidate lists (csrc/rt_cell_resolve.h: a pool of 64-byte records of 32 leaf slots for the
lists that keep 9 to 32 survivors under the sharper rule), checked on the CPU through the host model, with the probe of
test_cell_resolve_host.py plus two entry points.  Every list is forced to the overflow marker first.

Behaviour, on fans of level panes over the receiver quad and sphere of test_cell_resolve_host.py: 12 panes give a record that
lists exactly those 12 with entry 0 still the marker; 32 give a record, 33 none and no mark; a pool of one record hands out
exactly one; lists with at most 8 survivors and every flags word are what the stage writes without a pool; the final lists
pass flags_cases.check_shape.

Soundness, zero tolerance, as in test_cell_resolve_host.py: a record holds what the stage's walk keeps, so a slot a record
leaves out must not be accepted by the literal float32 triangle test for any shadow ray from the cell's hull to the light's
cloud (same hit points, same light points).  The two unsound ablations of the stage (RT_RESOLVE_NEAR_CENTRE,
RT_RESOLVE_NO_INFLATE) write records that leave out too much, and the same check must catch each."""
import ctypes as C

import numpy as np
import pytest

import flags_cases
import test_cell_resolve_host as rh
from test_cell_resolve_host import FAN_BUDGET, FANS, FULL, NEAR_CENTRE, NO_INFLATE, centre_cells, fan_slots, host, kept_of, load
from test_cell_prune_host import END, OVERFLOW, soft_cfg
from test_scene_pack_host import ptr
from hslu_i.ba_raytracing.f2501_raytracer_amd import _abi

W, MARK = 32, 0xFFFD

PROBE = rh.PROBE + r'''
extern "C" {
// the host model over the listed cells with a pool of `cap` records ([cap][32], 64-byte aligned; nullptr: no pool): lists
// [n][n_lights][8] and flags [n] of those cells, in place; returns how many records were asked for
uint32_t probe_resolve_wide(const uint32_t* cells, uint32_t n, uint32_t mode, uint16_t* lists, uint16_t* flags, uint16_t* pool, uint32_t cap) {
  RtCellResolveArgs a = R;
  uint32_t asked = 0;
  a.cell.mode = mode, a.cell.flag_geo = g.flag_geo.data(), a.cell.n_cells = g.n_cells, a.cell.n_tri_cells = g.n_tri_cells;
  if (pool) a.wide = pool, a.wide_cap = cap, a.wide_count = &asked;
  const uint32_t nl = g.dev.n_lights;
  for (uint32_t i = 0; i < n; i++)
    rt_cell_resolve_cell(g.dev, (const char*)g.blob.data(), a, cells[i], lists + (size_t)i * nl * RT_PRUNE_LIST_SLOTS, flags + i, nullptr);
  return asked;
}
// ... and over every cell through rt_cell_resolve_packed
uint32_t probe_resolve_wide_packed(uint16_t* lists, uint16_t* flags, uint32_t n_cells, uint16_t* pool, uint32_t cap) {
  RtCellResolveArgs a = R;
  uint32_t asked = 0;
  a.cell.mode = RT_PRUNE_FULL, a.cell.lists = lists, a.cell.flags = flags, a.cell.n_cells = n_cells;
  a.wide = pool, a.wide_cap = cap, a.wide_count = &asked;
  rt_cell_resolve_packed(g, a);
  return asked;
}
uint32_t probe_wide_index(const uint16_t* w) { return rt_cell_wide_index(w); }
uint64_t probe_wide_pool_bytes(uint32_t n_cells, uint32_t n_lights, uint64_t left, uint32_t* cap) { return rt_cell_wide_pool_bytes(n_cells, n_lights, (size_t)left, cap); }
}
'''

# fans with more panes than test_cell_resolve_host.py's: level panes 6e-3 apart, each a little shorter than the one below
WIDE_FANS = {"fan_32": 32, "fan_33": 33}


def tall_fan(n):
    import dataclasses
    flat = rh._soup([([0.3, 0.3, 0], [0.4, 0, 0], [0, 0.4, 0])], spheres=[(0.5, 0.5, 0.06, 0.05)], lights=[rh.LIGHT])  # (the receivers of fan_scene)
    panes = [([-0.5, -0.5, 0.2 + 0.006 * i], [2.5 - 0.03 * i, 0.0, 0.0], [0.0, 2.5, 0.0]) for i in range(n)]
    v1, e1, e2 = (np.array([p[i] for p in panes], np.float32) for i in range(3))
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])  # noqa: E731
    return dataclasses.replace(flat, tri_v1=cat(flat.tri_v1, v1), tri_e1=cat(flat.tri_e1, e1), tri_e2=cat(flat.tri_e2, e2), tri_normal=cat(flat.tri_normal, nrm),
                               tri_material=cat(flat.tri_material, np.zeros(n, np.uint32))).contiguous()


for _name, _n in WIDE_FANS.items():
    host.CASES[_name] = (lambda n=_n: (soft_cfg(), tall_fan(n), None))


def fan_budget(name):
    return FAN_BUDGET if name in FANS else 48 * (2 + WIDE_FANS[name]) + 8192


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import os
    if not os.path.exists(rh.HIPCC):
        pytest.skip("no hipcc")
    lib = rh.build_probe(tmp_path_factory.mktemp("cell_wide_probe"), PROBE)
    lib.probe_wide_pool_bytes.restype = C.c_uint64
    lib.probe_wide_index.restype = lib.probe_resolve_wide.restype = lib.probe_resolve_wide_packed.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def loaded(probe):
    cache = {}

    def get(name, budget=_abi.RT_SCENE_BUDGET_DEFAULT):
        if (name, budget) not in cache:
            cache.clear()  # (the probe holds one packed scene)
            cache[name, budget] = load(probe, name, budget)
        return cache[name, budget]
    return get


def new_pool(cap):
    """[cap][32] uint16 at a 64-byte boundary, filled with a value no record holds"""
    raw = np.full(cap * W + 64, 0xABCD, np.uint16)
    off = (-raw.ctypes.data % 64) // 2
    return raw[off:off + cap * W].reshape(cap, W)


def resolve(probe, k, cells, mode=FULL, cap=None):
    """every list of `cells` set to the marker and resolved -> lists, flags, pool, records asked for (cap None: no pool)"""
    cells = np.ascontiguousarray(cells, np.uint32)
    nl = k.dev["n_lights"]
    lists = np.full((len(cells), nl, 8), END, np.uint16)
    lists[:, :, 0] = OVERFLOW
    flags = np.zeros(len(cells), np.uint16)
    pool = new_pool(cap) if cap is not None else None
    asked = probe.probe_resolve_wide(ptr(cells), C.c_uint32(len(cells)), C.c_uint32(mode), ptr(lists), ptr(flags), ptr(pool) if pool is not None else None,
                                     C.c_uint32(cap or 0))
    return lists, flags, pool, int(asked)


def records(probe, lists, pool, n_slots):
    """{(row, light): [slots]} of the wide lists; checks the mark's words and the record's form on the way"""
    out, seen = {}, set()
    for i, l in zip(*np.nonzero(lists[:, :, 0] == OVERFLOW)):
        w = np.ascontiguousarray(lists[i, l])
        at = probe.probe_wide_index(ptr(w))
        if w[1] != MARK:
            assert at == 0xFFFFFFFF
            continue
        assert at < len(pool) and at not in seen, "every wide list has a record of its own inside the pool"
        seen.add(at)
        assert list(w[4:]) == [END] * 4 and w[2] < 0x8000 and w[3] < 0x8000 and at == int(w[2]) | (int(w[3]) << 15), w
        rec = pool[at]
        n = int((rec != END).sum())
        assert 8 < n <= W and (rec[:n] < n_slots).all() and (rec[n:] == END).all() and len(set(rec[:n].tolist())) == n, rec
        out[int(i), int(l)] = rec[:n].tolist()
    assert (pool[sorted(set(range(len(pool))) - seen)] == 0xABCD).all(), "records nobody points to are not written"
    return out


def all_cells(k):
    return np.arange(k.n_cells, dtype=np.uint32)


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
def test_twelve_panes_give_a_record_of_exactly_those_twelve(probe, loaded):
    k = loaded("fan_between", FAN_BUDGET)
    between, _ = fan_slots(k, 12)
    lists, flags, pool, asked = resolve(probe, k, all_cells(k), cap=k.n_cells)
    recs = records(probe, lists, pool, k.dev["n_slots"])
    quad, sphere = centre_cells(probe, k)
    for c in quad + sphere:
        assert lists[c, 0, 0] == OVERFLOW and lists[c, 0, 1] == MARK and not flags[c] & 1, (c, lists[c, 0])
        assert len(recs[c, 0]) == 12 and set(recs[c, 0]) == between, (c, recs[c, 0])
    assert asked == len(recs) <= k.n_cells


@pytest.mark.parametrize("name", list(WIDE_FANS))
def test_a_full_record_and_one_survivor_too_many(probe, loaded, name):
    n = WIDE_FANS[name]
    k = loaded(name, fan_budget(name))
    between = set(np.nonzero(k.tri_id >= 2)[0].tolist())
    assert len(between) == n and k.dev["n_slots"] == n + 2, "one leaf slot per triangle"
    lists, flags, pool, asked = resolve(probe, k, all_cells(k), cap=k.n_cells)
    recs = records(probe, lists, pool, k.dev["n_slots"])
    quad, sphere = centre_cells(probe, k)
    for c in quad + sphere:
        kept = np.nonzero(kept_of(probe, k, c)[0])[0].tolist()
        if c in sphere:
            assert set(kept) == between, "every pane, and nothing else, survives for the top of the sphere"
        if 8 < len(kept) <= W:
            assert lists[c, 0, 1] == MARK and sorted(recs[c, 0]) == kept, (c, lists[c, 0])
        else:  # (the quad's cells are its two whole triangles at this budget: they keep themselves as well)
            assert (c, 0) not in recs and lists[c, 0, 0] == OVERFLOW and lists[c, 0, 1] != MARK, lists[c, 0]
            assert list(lists[c, 0, 1:]) == [END] * 7, "a list that stays overflowed is not written"
    assert all(((c, 0) in recs) == (n <= W) for c in sphere)


def test_a_pool_of_one_record_hands_out_one(probe, loaded):
    k = loaded("fan_between", FAN_BUDGET)
    full, _, full_pool, _ = resolve(probe, k, all_cells(k), cap=k.n_cells)
    want = len(records(probe, full, full_pool, k.dev["n_slots"]))
    assert want > 1
    lists, flags, pool, asked = resolve(probe, k, all_cells(k), cap=1)
    recs = records(probe, lists, pool, k.dev["n_slots"])
    assert len(recs) == 1 and asked == want, "the counter runs on, the pool does not"
    over = lists[:, :, 0] == OVERFLOW
    assert int((over & (lists[:, :, 1] == MARK)).sum()) == 1
    plain = over & (lists[:, :, 1] != MARK)
    elsewhere = int(((full[:, :, 0] == OVERFLOW) & (full[:, :, 1] != MARK)).sum())  # (cells that are never looked up, lists above 32)
    assert int(plain.sum()) == want - 1 + elsewhere and (lists[plain][:, 1:] == END).all(), "the rest stays plain overflow, untouched"
    # through rt_cell_resolve_packed: same words, same single record
    l2 = np.full_like(lists, END)
    l2[:, :, 0] = OVERFLOW
    f2, p2 = np.zeros_like(flags), new_pool(1)
    assert probe.probe_resolve_wide_packed(ptr(l2), ptr(f2), C.c_uint32(k.n_cells), ptr(p2), C.c_uint32(1)) == want
    assert np.array_equal(l2, lists) and np.array_equal(f2, flags) and np.array_equal(p2, pool)


@pytest.mark.parametrize("name", list(FANS) + list(WIDE_FANS) + ["synthetic", "sphere_receiver"])
def test_short_lists_and_flags_are_those_of_the_stage_without_a_pool(probe, loaded, name):
    k = loaded(name, fan_budget(name) if name in FANS or name in WIDE_FANS else _abi.RT_SCENE_BUDGET_DEFAULT)
    cells = all_cells(k) if k.n_cells <= 4096 else np.asarray(k.cells, np.uint32)
    off_l, off_f, _, _ = resolve(probe, k, cells)
    on_l, on_f, pool, asked = resolve(probe, k, cells, cap=len(cells) * k.dev["n_lights"])
    recs = records(probe, on_l, pool, k.dev["n_slots"])
    wide = np.zeros(on_l.shape[:2], bool)
    for i, l in recs:
        wide[i, l] = True
    assert np.array_equal(on_f, off_f), "flag words"
    assert np.array_equal(on_l[~wide], off_l[~wide]), "every list that got no record, word for word"
    assert (off_l[wide][:, 0] == OVERFLOW).all(), "a record only where the stage left the marker"
    filled, over = flags_cases.check_shape(on_l, None, k.dev["n_slots"])
    print(f"{name}: {len(cells)} cells, {len(recs)} records, {filled} slots in short lists, {over} lists with the marker")
    # a record holds exactly what the walk keeps when it is offered every slot
    for (i, l), rec in list(recs.items())[:200]:
        kept = kept_of(probe, k, int(cells[i]))
        assert sorted(rec) == np.nonzero(kept[l])[0].tolist(), (int(cells[i]), l)


def test_the_pool_fits_its_bound(probe):
    for n_cells, nl, left in [(4096, 1, 1 << 20), (10_607_170, 5, 1 << 30), (10_607_170, 5, 1 << 40), (1, 1, 127), (1, 1, 128), (0, 5, 1 << 30), (3_000_000_000, 8, 1 << 50)]:
        cap = C.c_uint32(7)
        b = probe.probe_wide_pool_bytes(C.c_uint32(n_cells), C.c_uint32(nl), C.c_uint64(left), C.byref(cap))
        assert b <= left and (b == 0) == (cap.value == 0)
        if b:
            assert b == 64 * cap.value + 64 and cap.value <= -(-n_cells * nl // 8) and cap.value <= 1 << 30


# ---- soundness -----------------------------------------------------------------------------------------------------------------
def accepted_rays(probe, k, rng, c, l, s):
    pm, pt = host.hull_of(probe, c)
    so, d, tmax = host.shadow_rays(host.hit_points(rng, pm, pt), host.light_points(k, l, pm.astype(np.float64), k.isect[s]), k.cfg.eps_distance)
    valid, t = host.literal(k.isect[s], so, d)
    return int((valid & (t <= tmax)).sum()), len(so)


def left_out(probe, k, mode, beyond_full, cap, seed):
    """(cell, light, slot) triples the wide records written under `mode` leave out; beyond_full: only those the sound stage keeps"""
    cells = all_cells(k) if k.n_cells <= 4096 else np.asarray(k.cells, np.uint32)
    lists, _, pool, _ = resolve(probe, k, cells, mode=mode, cap=len(cells) * k.dev["n_lights"])
    recs = records(probe, lists, pool, k.dev["n_slots"])
    rng = np.random.default_rng(seed)
    triples, kept_cache = [], {}
    for (i, l), rec in recs.items():
        c = int(cells[i])
        if beyond_full:
            if c not in kept_cache:
                kept_cache[c] = kept_of(probe, k, c)
            out = sorted(set(np.nonzero(kept_cache[c][l])[0].tolist()) - set(rec))
        else:
            out = sorted(set(range(k.dev["n_slots"])) - set(rec))
        triples += [(c, l, s) for s in out]
    if len(triples) > cap:
        triples = [triples[i] for i in sorted(rng.choice(len(triples), cap, replace=False))]
    return len(recs), triples, rng


@pytest.mark.parametrize("name", list(FANS) + list(WIDE_FANS) + ["semesterbild"])
def test_no_slot_a_wide_record_leaves_out_is_accepted_by_any_shadow_ray(probe, loaded, name):
    k = loaded(name, fan_budget(name) if name != "semesterbild" else _abi.RT_SCENE_BUDGET_DEFAULT)
    n_recs, triples, rng = left_out(probe, k, FULL, False, 1500, seed=2)
    bad, rays = [], 0
    for c, l, s in triples:
        acc, n = accepted_rays(probe, k, rng, c, l, s)
        rays += n
        if acc:
            bad.append((c, l, s, acc))
    print(f"{name}: {n_recs} records, {len(triples)} left-out triples checked with {rays} rays, accepted {len(bad)}")
    if name not in ("fan_behind", "fan_mixed", "fan_33"):
        assert n_recs > 0 and triples, "there are wide records here, and they leave something out"
    assert not bad, f"left out of a record but accepted (cell, light, slot, rays): {bad[:10]}"


@pytest.mark.parametrize("what, mode", [("near side at the centre only", FULL | NEAR_CENTRE), ("no box inflation", FULL | NO_INFLATE)])
def test_a_record_that_leaves_out_too_much_is_caught(probe, loaded, what, mode):
    k = loaded("semesterbild")
    n_recs, triples, rng = left_out(probe, k, mode, True, 3000, seed=3)
    bad = [t for t in triples if accepted_rays(probe, k, rng, *t)[0]]
    print(f"{what}: {n_recs} records, {len(triples)} triples left out beyond the sound stage's, accepted by some ray: {len(bad)}")
    assert triples, "the ablation's records leave out more"
    assert bad, f"{what}: not caught at these sizes"
