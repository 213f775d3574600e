"""The kernels of ray orders (csrc/rt_order.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm UNIT=rt_order).  Every kernel exists, uses no scratch and spills nothing; no kernel waits for another workgroup;
and global memory sees no atomics (a wavefront adds one count per distinct digit, in LDS)."""
import os
import re

import pytest

import kernel_asm
from kernel_asm import CSRC

KERNELS = ("rt_order_bounds_kernel", "rt_order_frame_kernel", "rt_order_keys_kernel", "rt_order_hist_kernel", "rt_order_sums_kernel",
           "rt_order_tops_kernel", "rt_order_scan_kernel", "rt_order_scatter_kernel")


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    return kernel_asm.build("rt_order")


def test_every_order_kernel_is_built(build):
    remarks, bodies, descriptors = build
    assert set(remarks) == set(KERNELS), sorted(remarks)
    for name in KERNELS:
        assert name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_order_kernel_uses_no_scratch_and_spills_nothing(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name


def test_ranks_come_from_ballots_and_lds(build):
    """the rank inside a wavefront is a count of lanes below (mbcnt) in a ballot; counts meet in LDS, never in global atomics"""
    _, bodies, _ = build
    for name in ("rt_order_hist_kernel", "rt_order_scatter_kernel"):
        assert "v_mbcnt_hi_u32_b32" in bodies[name] and "v_mbcnt_lo_u32_b32" in bodies[name], name
    assert re.search(r"\bds_add_u32\b", bodies["rt_order_hist_kernel"])
    for name in KERNELS:
        assert not re.search(r"\b(global|flat)_atomic", bodies[name]), name
        assert "s_sleep" not in bodies[name], name  # no kernel waits for another workgroup


def test_sources_hold_no_inline_assembly():
    for f in ("rt_order.hip", "rt_ray_key.h", "rt_ray_order.cpp"):
        src = open(os.path.join(CSRC, f)).read().lower()
        assert "asm(" not in src and "asm volatile" not in src, f
