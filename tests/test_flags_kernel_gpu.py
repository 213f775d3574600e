"""rt_flags_kernel (csrc/rt_kernels.hip) on the GPU, its raw lists and flags held from both sides to references that never call
it (flags_cases.py), per (receiver cell, light):

  slots the literal triangle test accepts for some shadow ray from the cell            (soundness, zero tolerance)
    <=  slots the kernel lists, or its list is marked overflowed
    <=  slots the float64 restatement of the fat-beam rule does not clearly reject     (tightness; the near band is skipped)

and likewise the sphere bit against the sphere literal test and the f64 reach test.  Further: the shape of every list and
flags word of a scene, flags without lists == flags with lists, known answers under a small occluder, and two single-term
ablations of the f64 rule that the kernel's words contradict.  The probe links against the built librt_hip.so: the kernel
driven here is the one that ships."""
import numpy as np
import pytest

import f64_fat_beam as fb
import flags_cases as fc

pytestmark = pytest.mark.skipif(not fc.have_hipcc(), reason="no hipcc")
_runs = {}


def run(name):
    """(raw lists, raw flags, raw flags of the run without lists) of a scene, once per session"""
    if name not in _runs:
        k = fc.case(name)
        gpu = fc.gpu_probe()
        lists, flags = fc.run_flags(gpu, k, 1)
        _, flags0 = fc.run_flags(gpu, k, 0)
        _runs[name] = (lists, flags, flags0)
    return _runs[name]


def listed(row):
    return [int(s) for s in row if s < fc.OVERFLOW]


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.SCENES)
def test_lists_and_flags_hold_what_the_literal_tests_accept(name):
    R = fc.reference(name)
    lists, flags, _ = run(name)
    missing, not_clear, sphere_bit = [], [], []
    n_acc = 0
    for (c, l), acc in R.accepted.items():
        n_acc += len(acc)
        if acc and lists[c, l, 0] != fc.OVERFLOW:
            missing += [(c, l, s) for s in sorted(acc - set(listed(lists[c, l])))]
        if acc and flags[c] >> l & 1:
            not_clear.append((c, l))
        if R.sphere_hit[c, l] and flags[c] >> (8 + l) & 1:
            sphere_bit.append((c, l))
    print(f"{name}: {len(R.accepted)} (cell, light), {n_acc} literal-accepted slots, {sum(R.sphere_hit.values())} with a sphere hit; "
          f"missing {len(missing)}, triangle bits wrongly set {len(not_clear)}, sphere bits wrongly set {len(sphere_bit)}")
    assert not missing, f"accepted by the literal test, not listed (cell, light, slot): {missing[:10]}"
    assert not not_clear, f"a slot is accepted, the bit says no triangle can shadow the cell (cell, light): {not_clear[:10]}"
    assert not sphere_bit, f"a shadow ray meets a sphere, the bit says none can (cell, light): {sphere_bit[:10]}"


def tightness(R, lists, flags, clear=None, sph=None):
    """-> (listed slots the rule clearly rejects, overflowed lists with fewer than 9 kept-or-near slots, sphere bits that
    contradict a clear verdict, listed slots, of them in the near band, kept-or-near slots, overflowed lists)"""
    clear = clear or R.clear
    sph = sph or R.sph
    loose, short, sphere, n_listed, n_near, n_kept, n_over = [], [], [], 0, 0, 0, 0
    for (c, l), clr in clear.items():
        row = lists[c, l]
        kept = int((~clr).sum())
        n_kept += kept
        if row[0] == fc.OVERFLOW:
            n_over += 1
            if kept < 9:
                short.append((c, l, kept))
            row = row[1:]
        for s in listed(row):
            n_listed += 1
            if clr[s]:
                loose.append((c, l, s))
            elif (c, l) in R.rejected and R.rejected[c, l][s]:
                n_near += 1
        near, clearly_near, clearly_far = sph[c, l]
        bit = flags[c] >> (8 + l) & 1
        if (bit and clearly_near.any()) or (not bit and clearly_far.all()):
            sphere.append((c, l))
    return loose, short, sphere, n_listed, n_near, n_kept, n_over


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.SCENES)
def test_lists_and_flags_hold_nothing_the_f64_rule_clearly_rejects(name):
    R = fc.reference(name)
    lists, flags, _ = run(name)
    loose, short, sphere, n_listed, n_near, n_kept, n_over = tightness(R, lists, flags)
    rej, near = fc.near_share(R)
    print(f"{name}: f64 rule on {len(R.f64_cells)} cells: listed {n_listed} slots (kept or near {n_kept}), of them in the near band {n_near}; overflowed lists {n_over}; "
          f"near band {near} of {rej} rejected triples ({100.0 * near / max(rej, 1):.3f} %)")
    assert near <= fc.NEAR_CAP * rej
    assert not loose, f"listed, clearly rejected by the rule (cell, light, slot): {loose[:10]}"
    assert not short, f"marked overflowed with fewer than 9 kept-or-near slots (cell, light, kept): {short[:10]}"
    assert not sphere, f"sphere bit contradicts a clear verdict (cell, light): {sphere[:10]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.SCENES + fc.KNOWN)
def test_shape_of_every_list_and_flags_word_and_both_paths(name):
    k = fc.case(name)
    lists, flags, flags0 = run(name)
    n_listed, n_over = fc.check_shape(lists, flags, k.dev["n_slots"], k.active)
    print(f"{name}: {k.n_cells} cells, {int(k.active.sum())} active; listed slots {n_listed}, overflowed lists {n_over}, "
          f"triangle-clear bits {int(sum(bin(int(v) & 0xFF).count('1') for v in flags))}, sphere-clear bits {int(sum(bin(int(v) >> 8).count('1') for v in flags))}")
    assert n_listed + n_over > 0, "rt_flags_kernel listed something"
    # the walk returns early without lists (every cell of the wavefront has a survivor) and must not change a verdict
    assert np.array_equal(flags0, flags), f"{int((flags0 != flags).sum())} flags words differ between lists off and lists on"


def known_regions(k):
    """floor cells of the known-answers scene: far (hull more than 0.25, Chebyshev, from the middle) and under (hull inside
    |x - 0.5|, |y - 0.5| < 0.04); the occluder's slots and the floor's"""
    far, under, floor = [], [], []
    for c in range(k.n_cells):
        if not k.active[c] or abs(k.hulls[c][0][2]) > 1e-6:
            continue
        d = np.abs(k.hulls[c][1][:, :2].astype(np.float64) - 0.5).max(1)
        floor.append(c)
        if d.min() > 0.25:
            far.append(c)
        if d.max() < 0.04:
            under.append(c)
    occ = [s for s in range(k.dev["n_slots"]) if k.tri_id[s] >= 2]
    return far, under, floor, occ, [s for s in range(k.dev["n_slots"]) if k.tri_id[s] < 2]


# The known answers are asked of two packings of the one scene, each where the f64 rule decides them by 10 x the near band (the
# test below, on the CPU).  The rule's slack grows with the cell: with 23 x 23 floor cells it is too wide to clear every far
# cell without the box walk, which the f64 rule does not model; with 89 x 89 it is narrow enough to tell the occluder's two
# triangles apart under it, and a cell off the diagonal rightly lists one.
#   fine (89 x 89):   cells far from the occluder are clear, with empty lists
#   coarse (23 x 23): the cell under the occluder (one, astride the diagonal) lists exactly the occluder's two slots
#   both:             no floor cell lists a floor slot
def known_checks(name):
    k = fc.case(name)
    far, under, floor, occ, floor_slots = known_regions(k)
    assert len(occ) == 2 and len(floor_slots) == 2 and len(under) >= 1 and len(far) > 100, (name, len(far), len(under), occ, floor_slots)
    return k, (far if name == "known_answers_fine" else []), (under if name == "known_answers" else []), floor, occ, floor_slots


@pytest.mark.parametrize("name", fc.KNOWN)
def test_known_answer_regions_are_decided_by_ten_times_the_slack(name):
    """on the CPU: what the GPU test below expects of the kernel is what the f64 rule says, by at least 10 x the near band"""
    k, far, under, floor, occ, floor_slots = known_checks(name)
    for c in floor:
        B = fc.beam_of(k, c, 0)
        clearly_rejected = fb.triangles(B, k.isect, near=10 * fb.NEAR)[1]
        clearly_kept = ~fb.triangles(B, k.isect, near=-10 * fb.NEAR)[1]
        assert clearly_rejected[floor_slots].all(), c
        assert c not in far or clearly_rejected.all(), c
        assert c not in under or clearly_kept[occ].all(), c


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.KNOWN)
def test_known_answers_under_a_small_occluder(name):
    k, far, under, floor, occ, floor_slots = known_checks(name)
    lists, flags, _ = run(name)
    for c in far:
        assert flags[c] & 1 and (lists[c, 0] == fc.END).all(), f"cell {c}, far from the occluder: clear, empty list"
    for c in under:
        assert sorted(listed(lists[c, 0])) == sorted(occ) and not flags[c] & 1, f"cell {c}, under the occluder: exactly its two slots"
    for c in floor:
        assert lists[c, 0, 0] != fc.OVERFLOW and not set(listed(lists[c, 0])) & set(floor_slots), f"floor cell {c} lists a floor slot"
    assert all(flags[c] >> 8 & 1 for c in floor), "no sphere in the scene: the sphere bit is set"


ABLATIONS = {"no fb.r in delta": (dict(drop_r=True), {}), "t-rejection at the centre only": ({}, dict(centre_only=True))}


@pytest.mark.gpu
@pytest.mark.parametrize("ablation", list(ABLATIONS))
def test_a_single_term_ablation_of_the_f64_rule_contradicts_the_kernel(ablation):
    """the f64 rule with one term changed (computed on the CPU) no longer brackets what the kernel wrote: it clearly rejects
    slots the kernel lists (tightness fails), or slots the literal test accepts (soundness fails) -- the scenes can see such a
    mistake in the kernel too"""
    beam_kw, tri_kw = ABLATIONS[ablation]
    caught = {}
    for name in ("behind_and_through", "grazing", "ragged", "sphere_edges"):
        R = fc.reference(name)
        lists, flags, _ = run(name)
        clear = {(c, l): fb.triangles(fc.beam_of(R.k, c, l, **beam_kw), R.k.isect, **tri_kw)[1] for (c, l) in R.clear}
        loose = tightness(R, lists, flags, clear)[0]
        unsound = fc.unsound(R, clear)
        if loose or unsound:
            caught[name] = (len(loose), len(unsound))
    print(f"{ablation}: (listed but clearly rejected, accepted but clearly rejected) per scene: {caught}")
    assert caught, "no scene sees the mistake"
