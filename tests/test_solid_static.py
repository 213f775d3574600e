"""The kernel of the containment and signed-distance queries (csrc/rt_solid.hip) checked on the CPU: hipcc cross-compiles gfx950
here, with the Makefile's flags.  The kernel exists; it uses no scratch, spills no register, allocates no LDS and has no atomic;
no float operation is packed; the sources hold no inline assembly; and no loop ends in the EXEC-narrowing form beyond the one the
docstring of its test accounts for.  The register count and the occupancy are printed, not pinned: profiles/signed_distance.md
records what `make asm UNIT=rt_solid` reports."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, divergent_loops

KERNEL = "rt_solid_kernel"


@pytest.fixture(scope="module")
def build():
    """kernel_asm.compiled hands out the units it knows by name; rt_solid is a new unit of the same Makefile rule, named for the
    length of this one call only (as tests/test_multihit_static.py does)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernel_asm, "UNITS", tuple(kernel_asm.UNITS) + ("rt_solid",))
        c = kernel_asm.compiled("rt_solid")
    return c.remarks, c.bodies, c.descriptors


def test_the_kernel_exists(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == {KERNEL} == set(bodies) == set(descriptors), (sorted(remarks), sorted(bodies))
    assert "s_endpgm" in bodies[KERNEL]
    assert "global_load_dword" in bodies[KERNEL]  # per-lane vector loads: every lane walks for itself
    # the direction table and the plane pointers come from the kernel-argument segment where they are used
    assert re.search(r"\bs_load_dword", bodies[KERNEL])


def test_no_scratch_no_spills_no_lds_no_atomics(build):
    remarks, bodies, descriptors = build
    r = remarks[KERNEL]
    print(KERNEL, r)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[KERNEL])
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[KERNEL])
    assert not re.search(r"\bv_(write|read)lane_b32", bodies[KERNEL])  # (what a spilled scalar register would go through)
    assert not re.search(r"\b\w*atomic\w*", bodies[KERNEL]) and "s_sleep" not in bodies[KERNEL]
    assert not re.search(r"\bds_\w+", bodies[KERNEL]) and r["LDS Size [bytes/block]"] == 0
    # recorded, not pinned
    print("VGPRs %d, waves per SIMD %d" % (r["VGPRs"], r["Occupancy [waves/SIMD]"]))
    assert r["Occupancy [waves/SIMD]"] >= 1


def test_stores_are_plain_vector_stores(build):
    """one byte each for inside and votes, one dword per row entry and for the signed distance"""
    _, bodies, _ = build
    stores = set(re.findall(r"\b(?:global|flat)_store_\w+", bodies[KERNEL]))
    assert stores and stores <= {"global_store_byte", "global_store_dword", "global_store_short", "global_store_dwordx2", "global_store_dwordx3",
                                 "global_store_dwordx4"}, stores
    assert "global_store_byte" in stores and "global_store_dword" in stores


def test_no_packed_float_math(build):
    """the fused multiply-adds of the definition (dot products) and of the division and square-root sequences are v_fma_f32 /
    v_fmac_f32; nothing is paired into v_pk_*"""
    _, bodies, _ = build
    assert not re.search(r"\bv_pk_\w+", bodies[KERNEL])
    assert re.search(r"\bv_fmac?_f32", bodies[KERNEL]) and re.search(r"\bv_div_fixup_f32", bodies[KERNEL]) and re.search(r"\bv_sqrt_f32", bodies[KERNEL])
    assert not re.search(r"\bv_rsq_|\bv_mad_f32|\bv_mac_f32", bodies[KERNEL])


def test_sources_hold_no_inline_assembly():
    for f in ("rt_solid.hip", "rt_solid.h", "rt_solid.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f
        assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", src), f  # (no atomic call either)


def test_at_most_one_loop_narrows_exec(build):
    """Every loop of the kernel is controlled by a wave vote (RT_MH_ANY) or by scalars.  By scalars: the grid-stride loop over the
    batch, the sphere loop and the loop over the R directions.  By votes: the box-to-box stepping loop and the outer turn loop of
    the threaded walk.  The outer turn loop -- "evaluate one slot, step on" -- is the one the structuriser ends in the
    EXEC-narrowing form (s_andn2_b64 exec + s_cbranch_execz) in rt_multihit_kernel and rt_closest_kernel too: the check of
    tests/test_isa_invariants.py, with the bound those two kernels have.  A second one would mean some loop branches on a lane's
    own value."""
    _, bodies, _ = build
    assert divergent_loops(bodies[KERNEL]) <= 1
