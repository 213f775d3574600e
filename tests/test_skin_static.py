"""The kernels of skinned meshes (csrc/rt_skin.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm UNIT=rt_skin).  The three kernels exist, use no scratch, no LDS and no atomics, spill nothing and contain no loop
(the influence loop is unrolled); the vertex kernel and the vertex-normal triangle kernel contain no fused or packed float
instruction.  The face kernel is exempt from that one check: its normal is specified with two fma, a division and a square
root.  Nothing else about the instruction stream is asserted."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, loops_and_exits

KERNELS = ("rt_skin_vertex_kernel", "rt_skin_triangle_kernel", "rt_skin_face_kernel")
UNFUSED = ("rt_skin_vertex_kernel", "rt_skin_triangle_kernel")


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_skin")


def test_the_three_kernels_are_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]
        assert re.search(r"\bglobal_load_dword", bodies[name]) and re.search(r"\bglobal_store_dword", bodies[name]), name


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_uses_no_scratch_no_lds_no_atomics_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert remarks[name]["LDS Size [bytes/block]"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic|\bds_", bodies[name]), name
    assert "s_sleep" not in bodies[name] and "s_barrier" not in bodies[name], name


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_has_no_loop(build, name):
    """the four influences are unrolled; every branch only skips a block"""
    _, bodies, _ = build
    loops = loops_and_exits(bodies[name])
    print(name, [(len(m), e) for m, e in loops])
    assert loops == []


@pytest.mark.parametrize("name", UNFUSED)
def test_kernel_has_no_fused_or_packed_float_instruction(build, name):
    """w T_b(v), acc + w T_b(v), V[i1] - V[i0] and the two lerps are single multiplies and adds"""
    _, bodies, _ = build
    fused = re.findall(FUSED, bodies[name])
    assert not fused, sorted(set(fused))


def test_sources_hold_no_inline_assembly():
    for f in ("rt_skin.hip", "rt_skin.h", "rt_skin.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
