"""The kernels of the multi-hit ray queries (csrc/rt_multihit.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the
Makefile's flags.  Both list classes exist; neither uses scratch, spills a register, touches LDS or has an atomic; no float
operation is packed; the sources hold no inline assembly; and one loop, which the docstring of its test accounts for, ends in
the EXEC-narrowing form.  The register counts are printed and pinned to what `make asm UNIT=rt_multihit` reports
(profiles/multi_hit.md records them)."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, divergent_loops

# list class -> (VGPRs, waves per SIMD, LDS bytes) as measured
KERNELS = {"rt_multihit_kernel_k4": (65, 7, 0), "rt_multihit_kernel_k16": (101, 4, 0)}


@pytest.fixture(scope="module")
def build():
    """kernel_asm.compiled hands out the units it knows by name; rt_multihit is a new unit of the same Makefile rule, named for the
    length of this one call only (as tests/test_closest_static.py does)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernel_asm, "UNITS", tuple(kernel_asm.UNITS) + ("rt_multihit",))
        c = kernel_asm.compiled("rt_multihit")
    return c.remarks, c.bodies, c.descriptors


def test_the_kernels_exist(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS) == set(bodies) == set(descriptors), (sorted(remarks), sorted(bodies))
    for k in KERNELS:
        assert "s_endpgm" in bodies[k]
        assert "global_load_dword" in bodies[k]  # per-lane vector loads: every lane walks for itself


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_no_lds_no_atomics(build, kernel):
    remarks, bodies, descriptors = build
    r = remarks[kernel]
    print(kernel, r)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[kernel])
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[kernel])
    assert not re.search(r"\bv_(write|read)lane_b32", bodies[kernel])  # (what a spilled scalar register would go through)
    assert not re.search(r"\b\w*atomic\w*", bodies[kernel]) and "s_sleep" not in bodies[kernel]
    assert not re.search(r"\bds_", bodies[kernel])
    vgprs, waves, lds = KERNELS[kernel]
    assert (r["VGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, waves, lds)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_packed_float_math(build, kernel):
    """the fused multiply-adds of the definition (dot products, the discriminant, Ray::at) and of the division and square-root
    sequences are v_fma_f32 / v_fmac_f32; nothing is paired into v_pk_*"""
    _, bodies, _ = build
    assert not re.search(r"\bv_pk_\w+", bodies[kernel])
    assert re.search(r"\bv_fmac?_f32", bodies[kernel]) and re.search(r"\bv_div_fixup_f32", bodies[kernel]) and re.search(r"\bv_sqrt_f32", bodies[kernel])
    assert not re.search(r"\bv_rsq_|\bv_mad_f32|\bv_mac_f32", bodies[kernel])


def test_sources_hold_no_inline_assembly():
    for f in ("rt_multihit.hip", "rt_multihit.h", "rt_multihit.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f
        assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", src), f  # (no atomic call either)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_one_loop_narrows_exec(build, kernel):
    """Every loop of the kernel is controlled by a wave vote (RT_MH_ANY) or by scalars.  By scalars: the grid-stride loop, the
    pass loop's bound, the sphere loop, the two loops that shift the front keys in and out, and the loop over the max_hits
    entries of a row.  By votes: the pass loop ("some lane's list came back full"), the box-to-box stepping loop and the outer
    turn loop of the threaded walk.  The ONE loop the compiler ends in the EXEC-narrowing form (s_andn2_b64 exec +
    s_cbranch_execz) is that outer turn loop -- "evaluate one slot, step on" -- whose exit is the vote "no lane has a slot
    left": its structuriser routes that break through EXEC, though all lanes leave it together; rt_closest_kernel's walk has the
    same one.  A second one would mean some loop branches on a lane's own value."""
    _, bodies, _ = build
    assert divergent_loops(bodies[kernel]) <= 1
