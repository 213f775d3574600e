"""The kernels of a PLOC rebuild (csrc/rt_ploc.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm UNIT=rt_ploc).  Every kernel exists, uses no scratch and spills nothing; the distance's floats come from plain
multiplies and adds, never from a fused or packed form; no kernel waits for another workgroup; and the sources hold no
inline assembly."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED

KERNELS = ("rt_ploc_leaves_kernel", "rt_ploc_nearest_kernel", "rt_ploc_flags_kernel", "rt_ploc_merge_kernel", "rt_ploc_climb_kernel",
           "rt_ploc_gather_kernel", "rt_ploc_emit_kernel")
SOURCES = ("rt_ploc.hip", "rt_ploc.h", "rt_rebuild.cpp")
COUNTING = ("rt_ploc_climb_kernel", "rt_ploc_emit_kernel")  # leaves, the depth histogram, the cursors of the plan's groups


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_ploc")


def test_every_ploc_kernel_is_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_uses_no_scratch_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    # the neighbour search alone uses LDS: 6 planes of 256 + 2 * 32 floats
    assert remarks[name]["LDS Size [bytes/block]"] == (6 * (256 + 64) * 4 if name == "rt_ploc_nearest_kernel" else 0), name


def test_distances_and_boxes_have_no_fused_or_packed_float_form(build):
    """d = ex ey + ey ez + ez ex: three v_mul_f32 and two v_add_f32 per evaluation, extents from v_sub_f32 / v_add_f32; the pad of
    a leaf box likewise.  No kernel of the file holds a fused multiply-add or a packed float instruction at all."""
    _, bodies, _ = build
    for name in KERNELS:
        assert not re.findall(FUSED, bodies[name]), (name, re.findall(FUSED, bodies[name]))
    near = bodies["rt_ploc_nearest_kernel"]
    assert re.search(r"\bv_mul_f32", near) and re.search(r"\bv_add_f32", near) and re.search(r"\bds_read", near)


def test_no_kernel_waits_for_another_workgroup(build):
    """a launch boundary is the only ordering: no kernel sleeps or polls memory, there is no compare-and-swap, and only the two
    counting kernels hold an atomic at all"""
    _, bodies, _ = build
    for name in KERNELS:
        assert "s_sleep" not in bodies[name] and not re.search(r"\b(global|flat|ds)_(atomic_)?cmpswap|\b(global|flat)_atomic_cmpswap", bodies[name]), name
        if name not in COUNTING:
            assert not re.search(r"\b(global|flat)_atomic", bodies[name]), name
    for name in COUNTING:
        assert set(re.findall(r"\b(?:global|flat)_atomic_(\w+?)(?:_u32|_x2)?\b", bodies[name])) <= {"add", "umax", "inc"}, name


def test_sources_hold_no_inline_assembly():
    for f in SOURCES:
        src = open(os.path.join(CSRC, f)).read()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f
