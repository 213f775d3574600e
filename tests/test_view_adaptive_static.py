"""The kernels of adaptive camera views (csrc/rt_view_adapt.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with
the Makefile's flags (make asm UNIT=rt_view_adapt).  Held to the bar tests/test_view_static.py sets for the view kernels: every
kernel exists, uses no scratch and spills nothing; its VGPRs allow 8 waves per SIMD (at most 64: streaming kernels that hide
memory latency with occupancy); no loop ends on a per-lane condition; the float results of the classify and the resolve come
from single multiplies and adds.  What differs from the view kernels is stated per kernel: the partition ranks across the
four wavefronts of a workgroup through 16 bytes of LDS, and the classify adds one word per wavefront with one atomic."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC, FUSED, loops_and_exits

KERNELS = ("rt_view_classify_kernel", "rt_view_sparse_rays_kernel", "rt_view_flags_kernel", "rt_partition_count_kernel",
           "rt_partition_scatter_kernel", "rt_view_resolve_adaptive_kernel")
LDS_BYTES = {"rt_partition_count_kernel": 16, "rt_partition_scatter_kernel": 16}  # one count per wavefront of the workgroup
MAX_VGPRS = 64  # 512 / 64 = 8 waves per SIMD


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_view_adapt")


def test_all_adaptive_kernels_are_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_uses_no_scratch_spills_nothing_and_fits_eight_waves(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert remarks[name]["VGPRs"] <= MAX_VGPRS and remarks[name]["Occupancy [waves/SIMD]"] == 8
    assert remarks[name]["LDS Size [bytes/block]"] == LDS_BYTES.get(name, 0)
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name
    assert "s_sleep" not in bodies[name], name
    atomics = re.findall(r"\b(?:global|flat|ds)_atomic\w*", bodies[name])
    if name == "rt_view_classify_kernel":
        # one add per wavefront to the refined count; a vector instruction that returns nothing
        assert len(atomics) == 1 and atomics[0].startswith("global_atomic_add") and "sc0" not in [ln for ln in bodies[name].splitlines() if atomics[0] in ln][0]
    else:
        assert not atomics, (name, atomics)


@pytest.mark.parametrize("name", ["rt_view_classify_kernel", "rt_view_resolve_adaptive_kernel"])
def test_rule_and_resolve_have_no_fused_or_packed_arithmetic(build, name):
    """t_p - t_q, depth_tol * min, c_p - c_q; c * scale, the sums of the packets and the pack's * 255: single operations"""
    _, bodies, _ = build
    fused = re.findall(FUSED, bodies[name])
    assert not fused, sorted(set(fused))
    assert not re.search(r"\bv_div_|\bv_rcp_f32", bodies[name]), name


def test_no_loop_ends_on_a_per_lane_condition(build):
    """Only the resolve loops (its sample loop, whose trip count is a kernel argument); every branch that can leave that loop is
    decided by a scalar compare.  The classify's 8 neighbours are unrolled; the partition has no loop."""
    _, bodies, _ = build
    loops = {name: loops_and_exits(bodies[name]) for name in KERNELS}
    print({name: [(len(m), e) for m, e in ls] for name, ls in loops.items()})
    for name in KERNELS:
        if name != "rt_view_resolve_adaptive_kernel":
            assert loops[name] == [], name
    assert len(loops["rt_view_resolve_adaptive_kernel"]) == 1
    for members, exits in loops["rt_view_resolve_adaptive_kernel"]:
        assert exits and all(e in ("s_cbranch_scc0", "s_cbranch_scc1") for e in exits), exits


def test_sources_hold_no_inline_assembly():
    for f in ("rt_view_adapt.hip", "rt_view_adapt.h", "rt_view_adapt.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
