"""The kernels of a device-side BVH rebuild (csrc/rt_rebuild.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the
Makefile's flags (make asm UNIT=rt_rebuild).  Every kernel exists, uses no scratch and spills nothing; the key kernel's floats come
from single multiplies, adds and one correctly rounded division per axis, never from a fused or packed form the source does
not name; no kernel waits for another workgroup; and the sources hold no inline assembly."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, division_steps

KERNELS = ("rt_lbvh_frame_kernel", "rt_lbvh_keys_kernel", "rt_lbvh_karras_kernel", "rt_lbvh_depth_kernel", "rt_lbvh_gather_kernel",
           "rt_lbvh_emit_kernel", "rt_lbvh_single_kernel")
SOURCES = ("rt_rebuild.hip", "rt_rebuild.cpp", "rt_lbvh.h")


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_rebuild")


def test_every_rebuild_kernel_is_built(build):
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
    assert "s_sleep" not in bodies[name], name


def test_key_kernel_has_no_fused_multiply_add_of_its_own(build):
    """centre = 0.5 (min + max) and cell = (c - lo) / extent * 1024: adds, multiplies and, once per axis, the compiler's
    correctly rounded division -- v_div_scale x 2, v_rcp, Newton steps fused by construction, v_div_fmas, v_div_fixup.
    Membership is decided by data flow (kernel_asm.division_steps): every fused instruction of the kernel is a step
    of one of the three divisions, and no packed float instruction exists.  The frame kernel divides nothing and fuses nothing."""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies["rt_lbvh_keys_kernel"].splitlines()]
    op = lambda ln: ln.split()[0] if ln else ""  # noqa: E731
    fmas = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fmas_f32")]
    assert len(fmas) == 3 and sum(op(ln).startswith("v_div_fixup_f32") for ln in lines) == 3, "one division per axis"
    fused = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(FUSED, ln)] if m]
    print("fused instructions of the key kernel:", [f for _, f in fused])
    assert all(re.fullmatch(r"v_fmac?_f32(_e32|_e64)?", f) for _, f in fused), fused
    divisions = [division_steps(lines, at) for at in fmas]
    for steps in divisions:
        kinds = sorted(re.sub(r"_e(32|64)$", "", op(lines[k])) for k in steps)
        assert kinds == sorted(["v_div_scale_f32"] * 2 + ["v_rcp_f32", "v_mul_f32"] + ["v_fma_f32"] * 3 + ["v_fmac_f32"] * 2), kinds
    inside = set().union(*divisions)
    outside = [(i, f) for i, f in fused if i not in inside]
    assert not outside, outside
    assert not re.findall(FUSED, bodies["rt_lbvh_frame_kernel"])


def test_no_kernel_waits_for_another_workgroup(build):
    """a launch boundary is the only ordering: no loop of any rebuild kernel sleeps or polls memory, and the atomics are
    counts -- adds and maxima, never a compare-and-swap"""
    _, bodies, _ = build
    for name in KERNELS:
        assert "s_sleep" not in bodies[name] and not re.search(r"\b(global|flat)_atomic_cmpswap", bodies[name]), name
    for name in ("rt_lbvh_frame_kernel", "rt_lbvh_keys_kernel", "rt_lbvh_karras_kernel", "rt_lbvh_gather_kernel", "rt_lbvh_single_kernel"):
        assert not re.search(r"\b(global|flat)_atomic", bodies[name]), name


def test_sources_hold_no_inline_assembly():
    for f in SOURCES:
        src = open(os.path.join(CSRC, f)).read()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f
