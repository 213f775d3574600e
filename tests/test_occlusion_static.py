"""The kernels of the ambient-occlusion queries (csrc/rt_occlusion.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with
the Makefile's flags.  Both classes exist; neither uses scratch, spills a register, allocates LDS or has an atomic; no float
operation is packed; the sources hold no inline assembly; and no loop ends in the EXEC-narrowing form beyond the one the
docstring of its test accounts for.  The register counts are printed and pinned to what `make asm UNIT=rt_occlusion` reports
(profiles/ambient_occlusion.md records them)."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, divergent_loops

# class -> (VGPRs, waves per SIMD, LDS bytes) as measured
KERNELS = {"rt_occlusion_kernel_s64": (49, 8, 0), "rt_occlusion_kernel_wide": (60, 8, 0)}


@pytest.fixture(scope="module")
def build():
    """kernel_asm.compiled hands out the units it knows by name; rt_occlusion is a new unit of the same Makefile rule, named for
    the length of this one call only (as tests/test_multihit_static.py does)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernel_asm, "UNITS", tuple(kernel_asm.UNITS) + ("rt_occlusion",))
        c = kernel_asm.compiled("rt_occlusion")
    return c.remarks, c.bodies, c.descriptors


def test_the_kernels_exist(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS) == set(bodies) == set(descriptors), (sorted(remarks), sorted(bodies))
    for k in KERNELS:
        assert "s_endpgm" in bodies[k]
        assert "global_load_dword" in bodies[k]  # per-lane vector loads: every lane walks for itself


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_no_lds_no_atomics(build, kernel):
    """The only ds_ instruction is ds_bpermute_b32, the cross-lane read of __shfl_xor in the butterfly of the three int32 sums:
    it goes through the LDS crossbar and touches no LDS memory, so the kernels allocate none."""
    remarks, bodies, descriptors = build
    r = remarks[kernel]
    print(kernel, r)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[kernel])
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[kernel])
    assert not re.search(r"\bv_(write|read)lane_b32", bodies[kernel])  # (what a spilled scalar register would go through)
    assert not re.search(r"\b\w*atomic\w*", bodies[kernel]) and "s_sleep" not in bodies[kernel]
    assert set(re.findall(r"\bds_\w+", bodies[kernel])) == {"ds_bpermute_b32"}
    vgprs, waves, lds = KERNELS[kernel]
    assert (r["VGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, waves, lds)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_packed_float_math(build, kernel):
    """the fused multiply-adds of the definition (the frame, the origin, the world direction, dot products, the discriminant) and
    of the division and square-root sequences are v_fma_f32 / v_fmac_f32; nothing is paired into v_pk_*"""
    _, bodies, _ = build
    assert not re.search(r"\bv_pk_\w+", bodies[kernel])
    assert re.search(r"\bv_fmac?_f32", bodies[kernel]) and re.search(r"\bv_div_fixup_f32", bodies[kernel]) and re.search(r"\bv_sqrt_f32", bodies[kernel])
    assert not re.search(r"\bv_rsq_|\bv_mad_f32|\bv_mac_f32", bodies[kernel])


def test_sources_hold_no_inline_assembly():
    for f in ("rt_occlusion.hip", "rt_occlusion.h", "rt_occlusion.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f
        assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", src), f  # (no atomic call either)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_at_most_one_loop_narrows_exec(build, kernel):
    """Every loop of the kernels is controlled by a wave vote (RT_MH_ANY) or by scalars.  By scalars: the grid-stride loop over
    groups of points (its index starts at a readfirstlane of the wave's number), the loop that halves seg down to the sample
    count, the rounds of the wide class, and the sphere loop, whose early end is the vote "no lane still asks".  By votes: the
    box-to-box stepping loop and the outer turn loop of the threaded walk.  The butterfly of the sums is unrolled.  The outer
    turn loop -- "evaluate one slot, step on" -- is the one rt_multihit_kernel's and rt_closest_kernel's structuriser ends in the
    EXEC-narrowing form (s_andn2_b64 exec + s_cbranch_execz); here a lane that found its hit has nothing left in the loop, and
    the compiler emits none.  A second one would mean some loop branches on a lane's own value."""
    _, bodies, _ = build
    assert divergent_loops(bodies[kernel]) <= 1
