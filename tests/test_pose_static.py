"""The kernels of part poses and of the SAH report (csrc/rt_pose.hip, csrc/rt_sah.hip) checked on the CPU: hipcc cross-compiles
gfx950 here, with the Makefile's flags (make asm UNIT=rt_pose, UNIT=rt_sah).  Both kernels exist, use no scratch and spill nothing; the pose
kernel's float results come from single multiplies and adds and one correctly rounded division, never from a fused or packed
form the source does not name; and no loop ends on a per-lane condition."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, division_steps, loops_and_exits

KERNELS = {"rt_pose_kernel": "pose", "rt_sah_kernel": "sah"}


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_pose", "rt_sah")


def test_both_kernels_are_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_kernel_uses_no_scratch_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    assert "s_sleep" not in bodies[name], name


def test_pose_kernel_is_plain_loads_and_stores(build):
    """no LDS, no atomics: one thread, one object"""
    remarks, bodies, _ = build
    body = bodies["rt_pose_kernel"]
    assert remarks["rt_pose_kernel"]["LDS Size [bytes/block]"] == 0
    assert not re.search(r"\b(global|flat|ds)_atomic|\bds_", body)
    assert re.search(r"\bglobal_load_dword", body) and re.search(r"\bglobal_store_dword", body)


def test_sah_kernel_adds_once_per_sum_and_workgroup(build):
    """three 64-bit atomic adds in the code (inner_q, leaf_q, n_bad: one lane each), behind the LDS reduction"""
    remarks, bodies, _ = build
    body = bodies["rt_sah_kernel"]
    atomics = re.findall(r"\b(?:global|flat)_atomic_\w+", body)
    print("atomics of the SAH kernel:", atomics)
    assert atomics and all(a.endswith("add_x2") for a in atomics) and len(atomics) <= 3, atomics
    assert "cmpswap" not in body
    assert 0 < remarks["rt_sah_kernel"]["LDS Size [bytes/block]"] <= 256
    assert "s_barrier" in body


def test_pose_kernel_fuses_nothing_outside_its_one_division(build):
    """1 / r' is the compiler's correctly rounded division: v_div_scale x 2, v_rcp, Newton steps fused by construction,
    v_div_fmas, v_div_fixup.  Membership is decided by data flow (kernel_asm.division_steps): every fused instruction
    of the kernel is a step of that division, and no packed float instruction exists."""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies["rt_pose_kernel"].splitlines()]
    op = lambda ln: ln.split()[0] if ln else ""  # noqa: E731
    fixups = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fixup_f32")]
    scales = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_scale_f32")]
    fmas = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fmas_f32")]
    assert len(fixups) == 1 and len(fmas) == 1 and len(scales) == 2, (len(fixups), len(fmas), len(scales))
    fused = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(FUSED, ln)] if m]
    print("fused instructions of the pose kernel:", [f for _, f in fused])
    assert all(re.fullmatch(r"v_fmac?_f32(_e32|_e64)?", f) for _, f in fused), fused
    steps = division_steps(lines, fmas[0])
    kinds = sorted(re.sub(r"_e(32|64)$", "", op(lines[k])) for k in steps)
    print("division:", [lines[k] for k in steps])
    assert kinds == sorted(["v_div_scale_f32"] * 2 + ["v_rcp_f32", "v_mul_f32"] + ["v_fma_f32"] * 3 + ["v_fmac_f32"] * 2), kinds
    outside = [(i, f) for i, f in fused if i not in steps]
    assert not outside, outside
    # the arithmetic that is there is the single forms
    assert sum(op(ln).startswith("v_mul_f32") for ln in lines) >= 40 and sum(op(ln).startswith(("v_add_f32", "v_sub_f32")) for ln in lines) >= 30


def test_sah_kernel_has_no_fused_double_arithmetic(build):
    """dx dy + dy dz + dz dx and ratio 2^30 are single fp64 multiplies and adds; the one fp64 division is the compiler's
    correctly rounded sequence (its Newton steps are v_fma_f64 by construction)"""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies["rt_sah_kernel"].splitlines()]
    ops = [ln.split()[0] for ln in lines if ln]
    assert any(o.startswith("v_mul_f64") for o in ops) and any(o.startswith("v_add_f64") for o in ops)
    assert not [o for o in ops if o.startswith("v_pk_")]
    assert not [o for o in ops if re.match(r"v_(fma|fmac|mad|mac)_f32", o)]
    n_div = sum(o.startswith("v_div_fmas_f64") for o in ops)
    assert n_div >= 1
    # every v_fma_f64 belongs to a division: none is left when the divisions' Newton steps are set aside (at most 7 each)
    assert sum(o.startswith("v_fma_f64") for o in ops) <= 7 * n_div


def test_no_loop_ends_on_a_per_lane_condition(build):
    """The pose kernel has no loop.  Whatever loop the SAH kernel keeps (its reductions have constant trip counts) is left on
    a scalar compare only."""
    _, bodies, _ = build
    loops = {name: loops_and_exits(bodies[name]) for name in KERNELS}
    print({name: [(len(m), e) for m, e in ls] for name, ls in loops.items()})
    assert loops["rt_pose_kernel"] == []
    for members, exits in loops["rt_sah_kernel"]:
        assert exits and all(e in ("s_cbranch_scc0", "s_cbranch_scc1") for e in exits), exits


def test_sources_hold_no_inline_assembly():
    for f in ("rt_pose.hip", "rt_pose.h", "rt_pose.cpp", "rt_sah.hip", "rt_sah.h"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
