"""The kernel of the closest-point queries (csrc/rt_closest.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the
Makefile's flags.  The kernel exists; it uses no scratch, spills nothing and has no LDS; every float result outside the
compiler's correctly rounded division and square-root sequences is a single multiply or add -- nothing contracted, nothing
packed -- which is what lets the kernel equal the host model bit for bit; the sources hold no inline assembly; and at most
one loop ends in the EXEC-narrowing form."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, division_steps, divergent_loops

KERNEL = "rt_closest_kernel"


@pytest.fixture(scope="module")
def build():
    """kernel_asm.compiled hands out the units it knows by name; rt_closest is a new unit of the same Makefile rule, named for the
    length of this one call only (as tests/test_view_lens_static.py does)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernel_asm, "UNITS", tuple(kernel_asm.UNITS) + ("rt_closest",))
        c = kernel_asm.compiled("rt_closest")
    return c.remarks, c.bodies, c.descriptors


def test_the_kernel_exists(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == {KERNEL} == set(bodies) == set(descriptors), (sorted(remarks), sorted(bodies))
    assert "s_endpgm" in bodies[KERNEL]
    assert "global_load_dword" in bodies[KERNEL]  # per-lane vector loads: every lane walks for itself


def test_no_scratch_no_spills_no_lds(build):
    remarks, bodies, descriptors = build
    print(KERNEL, remarks[KERNEL])
    r = remarks[KERNEL]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[KERNEL])
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[KERNEL])
    assert r["LDS Size [bytes/block]"] == 0 and not re.search(r"\bds_", bodies[KERNEL])
    assert not re.search(r"\b(?:global|flat)_atomic\w*", bodies[KERNEL]) and "s_sleep" not in bodies[KERNEL]
    assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8  # latency of the per-lane loads is hidden by occupancy


def test_nothing_fused_or_packed_outside_division_and_square_root(build):
    """A correctly rounded division is two v_div_scale, a reciprocal, Newton steps that are fused by construction, v_div_fmas and
    v_div_fixup (membership by data flow, kernel_asm.division_steps).  A correctly rounded square root is v_sqrt_f32 and two
    residuals r - s' * s, each a v_fma_f32 that reads the root.  Every other float result is a single multiply or add."""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies[KERNEL].splitlines()]
    op = lambda ln: ln.split()[0] if ln else ""  # noqa: E731
    regs = lambda ln: re.findall(r"\bv\d+\b", ln)  # noqa: E731
    fmas = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fmas_f32")]
    assert fmas and len([ln for ln in lines if op(ln).startswith("v_div_fixup_f32")]) == len(fmas)
    fused = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(FUSED, ln)] if m]
    assert all(re.fullmatch(r"v_fmac?_f32(_e32|_e64)?", f) for _, f in fused), sorted({f for _, f in fused})
    inside = set()
    for at in fmas:
        inside |= set(division_steps(lines, at))
    roots = [i for i, ln in enumerate(lines) if op(ln).startswith("v_sqrt_f32")]
    assert roots and not re.search(r"\bv_rsq_", bodies[KERNEL])
    for at in roots:
        root = regs(lines[at])[0]
        residuals = [k for k in range(at + 1, min(at + 12, len(lines))) if op(lines[k]) == "v_fma_f32" and root in regs(lines[k])[1:]]
        assert len(residuals) == 2, (lines[at], residuals)
        inside |= set(residuals)
    outside = [(i, lines[i]) for i, _ in fused if i not in inside]
    print(KERNEL, len(fmas), "divisions,", len(roots), "square roots,", len(fused), "fused instructions, outside:", outside)
    assert not outside, outside


def test_sources_hold_no_inline_assembly():
    for f in ("rt_closest.hip", "rt_closest.h", "rt_closest.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src and "__asm" not in src, f


def test_at_most_one_loop_narrows_exec(build):
    """Every loop of the kernel is controlled by a wave vote (RT_CLOSEST_ANY): the sphere loop and the grid-stride loop by scalars,
    the seed descent, the seed's leaf and the box-to-box stepping loop by ballots.  The ONE loop the compiler ends in the
    EXEC-narrowing form (s_andn2_b64 exec + s_cbranch_execz) is the outer turn loop of the threaded walk -- "evaluate one slot,
    step on" -- whose exit is the vote "no lane has a slot left": its structuriser routes that break through EXEC, though all lanes
    leave it together.  A second one would mean some loop branches on a lane's own value."""
    _, bodies, _ = build
    assert divergent_loops(bodies[KERNEL]) <= 1
