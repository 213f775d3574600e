"""The kernels of camera views (csrc/rt_view.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm UNIT=rt_view).  Both kernels exist, use no scratch and spill nothing; their float results come from single
multiplies, adds and correctly rounded divisions, never from a fused or packed form the source does not name; and no loop
ends on a per-lane condition."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, division_steps, loops_and_exits

KERNELS = ("rt_view_rays_kernel", "rt_view_resolve_kernel")


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_view")


def test_both_view_kernels_are_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_view_kernel_uses_no_scratch_no_lds_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert remarks[name]["LDS Size [bytes/block]"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    assert not re.search(r"\b(global|flat|ds)_atomic|\bds_(add|sub|inc|dec)", bodies[name]) and "s_sleep" not in bodies[name], name


def test_resolve_kernel_has_no_fused_or_packed_arithmetic(build):
    """c * scale, the sums of the packets and the pack's * 255 are single operations"""
    _, bodies, _ = build
    fused = re.findall(FUSED, bodies["rt_view_resolve_kernel"])
    assert not fused, sorted(set(fused))
    assert not re.search(r"\bv_div_|\bv_rcp_f32", bodies["rt_view_resolve_kernel"]), "the sample weight is computed on the host"


def test_rays_kernel_fuses_nothing_outside_its_two_divisions(build):
    """The generator divides twice (a and b, by the image height).  The compiler's correctly rounded division is a sequence
    v_div_scale x 2, v_rcp, Newton steps, v_div_fmas, v_div_fixup whose Newton steps are fused by construction; every other
    float result is a single multiply or add.  The scheduler interleaves the two sequences with each other and with the
    `* tan_half` that follows the first, so membership is decided by data flow, not by position: the steps of a division are
    what its v_div_fmas reads, back to its two v_div_scale.  Per division these are the two scales, one reciprocal, one
    multiply and five plain v_fma_f32 / v_fmac_f32 -- and no fused or packed instruction of the kernel lies outside them."""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies["rt_view_rays_kernel"].splitlines()]
    op = lambda ln: ln.split()[0] if ln else ""  # noqa: E731
    fixups = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fixup_f32")]
    scales = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_scale_f32")]
    fmas = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fmas_f32")]
    assert len(fixups) == 2 and len(fmas) == 2 and len(scales) == 4, (len(fixups), len(fmas), len(scales))
    fused = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(FUSED, ln)] if m]
    print("fused instructions of the generator:", [f for _, f in fused])
    assert all(re.fullmatch(r"v_fmac?_f32(_e32|_e64)?", f) for _, f in fused), fused
    divisions = [division_steps(lines, at) for at in fmas]
    for steps in divisions:
        kinds = sorted(re.sub(r"_e(32|64)$", "", op(lines[k])) for k in steps)
        print("division:", [lines[k] for k in steps])
        assert kinds == sorted(["v_div_scale_f32"] * 2 + ["v_rcp_f32", "v_mul_f32"] + ["v_fma_f32"] * 3 + ["v_fmac_f32"] * 2), kinds
    assert not set(divisions[0]) & set(divisions[1])
    outside = [(i, f) for i, f in fused if i not in divisions[0] and i not in divisions[1]]
    assert not outside, outside


def test_no_loop_ends_on_a_per_lane_condition(build):
    """The generator has no loop.  The resolve has its sample loop, whose trip count is a kernel argument: every branch that can
    leave it is decided by a scalar compare (s_cbranch_scc*), never by the execution mask or a vector compare
    (s_cbranch_execz / execnz / vccz / vccnz) -- those only skip blocks inside an iteration."""
    _, bodies, _ = build
    loops = {name: loops_and_exits(bodies[name]) for name in KERNELS}
    print({name: [(len(m), e) for m, e in ls] for name, ls in loops.items()})
    assert loops["rt_view_rays_kernel"] == []
    assert len(loops["rt_view_resolve_kernel"]) == 1
    for members, exits in loops["rt_view_resolve_kernel"]:
        assert exits and all(e in ("s_cbranch_scc0", "s_cbranch_scc1") for e in exits), exits


def test_sources_hold_no_inline_assembly():
    for f in ("rt_view.hip", "rt_view.h", "rt_view.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
