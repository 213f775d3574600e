"""The kernels of thin-lens camera views (csrc/rt_view_lens.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the
Makefile's flags.  Held to the bar tests/test_view_static.py sets for the view kernels and stating only what the design fixes:
the exact kernel set; no scratch, no spills; in the two generators and the coc kernel every float result is a single multiply,
add, correctly rounded division or correctly rounded square root -- nothing the compiler contracted; no loop ends on a per-lane
condition; LDS only in the spread kernel, whose one atomic is the per-workgroup add to the refined count."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, division_steps, loops_and_exits

KERNELS = ("rt_view_lens_rays_kernel", "rt_view_lens_sparse_rays_kernel", "rt_view_coc_kernel", "rt_view_defocus_spread_kernel")
SPREAD = "rt_view_defocus_spread_kernel"
# a and b divide by the image height in every kernel that makes a direction; the coc divides t by |d0| and by z F as well
DIVISIONS = {"rt_view_lens_rays_kernel": 2, "rt_view_lens_sparse_rays_kernel": 2, "rt_view_coc_kernel": 4}
TILE_BYTES = 4 * (16 + 2 * 16) ** 2  # 16 x 16 pixels and a halo of 16, the largest spread



@pytest.fixture(scope="module")
def build():
    """kernel_asm.compiled hands out the units it knows by name; the lens kernels are a new unit of the same Makefile rule, named
    for the length of this one call only (the record stays in compiled's cache; nothing outside this call sees another UNITS)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernel_asm, "UNITS", tuple(kernel_asm.UNITS) + ("rt_view_lens",))
        c = kernel_asm.compiled("rt_view_lens")
    return c.remarks, c.bodies, c.descriptors


def test_exactly_the_four_lens_kernels_are_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS) == set(bodies) == set(descriptors), (sorted(remarks), sorted(bodies))
    for name in KERNELS:
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_uses_no_scratch_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    assert "s_sleep" not in bodies[name], name
    assert remarks[name]["Occupancy [waves/SIMD]"] == 8  # streaming kernels: latency is hidden by occupancy


@pytest.mark.parametrize("name", KERNELS)
def test_lds_and_atomics_only_in_the_spread_kernel(build, name):
    remarks, bodies, _ = build
    lds = remarks[name]["LDS Size [bytes/block]"]
    atomics = re.findall(r"\b(?:global|flat|ds)_atomic\w*", bodies[name])
    if name == SPREAD:
        # the tile, and what the barrier's vote takes beside it
        assert TILE_BYTES <= lds <= TILE_BYTES + 1024, lds
        assert re.search(r"\bds_read", bodies[name]) and re.search(r"\bds_write", bodies[name])
        assert len(atomics) == 1 and atomics[0].startswith("global_atomic_add"), atomics
        assert "sc0" not in [ln for ln in bodies[name].splitlines() if atomics[0] in ln][0]  # (returns nothing)
    else:
        assert lds == 0 and not re.search(r"\bds_", bodies[name]) and not atomics, (name, lds, atomics)


@pytest.mark.parametrize("name", sorted(DIVISIONS))
def test_generators_and_coc_fuse_nothing_the_source_does_not_name(build, name):
    """The correctly rounded division is the sequence tests/test_view_static.py describes (two v_div_scale, a reciprocal, Newton
    steps that are fused by construction, v_div_fmas, v_div_fixup); membership is decided by data flow.  The correctly rounded
    square root of the coc kernel is v_sqrt_f32 and two residuals r - s * s', each a v_fma_f32 that reads the root.  Every other
    float result is a single multiply or add: no fused or packed instruction lies outside those sequences."""
    _, bodies, _ = build
    lines = [ln.strip() for ln in bodies[name].splitlines()]
    op = lambda ln: ln.split()[0] if ln else ""  # noqa: E731
    fmas = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fmas_f32")]
    fixups = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_fixup_f32")]
    scales = [i for i, ln in enumerate(lines) if op(ln).startswith("v_div_scale_f32")]
    n = DIVISIONS[name]
    assert (len(fmas), len(fixups), len(scales)) == (n, n, 2 * n), (len(fmas), len(fixups), len(scales))
    fused = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(FUSED, ln)] if m]
    print(name, "fused instructions:", [f for _, f in fused])
    assert all(re.fullmatch(r"v_fmac?_f32(_e32|_e64)?", f) for _, f in fused), fused
    divisions = [division_steps(lines, at) for at in fmas]
    inside = set()
    for steps in divisions:
        kinds = sorted(re.sub(r"_e(32|64)$", "", op(lines[k])) for k in steps)
        assert kinds == sorted(["v_div_scale_f32"] * 2 + ["v_rcp_f32", "v_mul_f32"] + ["v_fma_f32"] * 3 + ["v_fmac_f32"] * 2), kinds
        assert not inside & set(steps)
        inside |= set(steps)
    outside = [(i, f) for i, f in fused if i not in inside]
    roots = [ln for ln in lines if op(ln).startswith("v_sqrt_f32")]
    assert not re.search(r"\bv_rsq_", bodies[name])  # (v_rcp_iflag_f32 is the integer division p / width)
    if name != "rt_view_coc_kernel":
        assert not roots and not outside, (roots, outside)
        return
    assert len(roots) == 1, roots
    root = re.findall(r"\bv\d+\b", roots[0])[0]
    assert len(outside) == 2, outside
    for i, f in outside:
        assert f == "v_fma_f32" and root in re.findall(r"\bv\d+\b", lines[i])[1:], lines[i]


def test_no_loop_ends_on_a_per_lane_condition(build):
    """The generators and the coc kernel have no loop.  The spread kernel loops over the cells of its tile and over its window;
    both trip counts come from `spread`, a kernel argument: every branch that can leave a loop is decided by a scalar compare."""
    _, bodies, _ = build
    loops = {name: loops_and_exits(bodies[name]) for name in KERNELS}
    print({name: [(len(m), e) for m, e in ls] for name, ls in loops.items()})
    for name in KERNELS:
        if name != SPREAD:
            assert loops[name] == [], name
    assert loops[SPREAD]
    for members, exits in loops[SPREAD]:
        assert exits and all(e in ("s_cbranch_scc0", "s_cbranch_scc1") for e in exits), exits
    assert kernel_asm.divergent_loops(bodies[SPREAD]) == 0


def test_sources_hold_no_inline_assembly():
    for f in ("rt_view_lens.hip", "rt_view_lens.h", "rt_view_lens.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
