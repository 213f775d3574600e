"""The kernels of ray orders (csrc/rt_order.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm-order).  Every kernel exists, uses no scratch and spills nothing; no kernel waits for another workgroup;
and global memory sees no atomics (a wavefront adds one count per distinct digit, in LDS)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ("rt_order_bounds_kernel", "rt_order_frame_kernel", "rt_order_keys_kernel", "rt_order_hist_kernel", "rt_order_sums_kernel",
           "rt_order_tops_kernel", "rt_order_scan_kernel", "rt_order_scatter_kernel")


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("order_asm") / "rt_order.s"
    r = subprocess.run(["make", "-C", CSRC, "asm-order", "ORDER_ASM_OUT=" + str(asm)], check=True, capture_output=True, text=True, timeout=900)
    remarks = {}
    for block in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(rt_order_[a-z]+_kernel)E", block)
        if m:
            remarks[m.group(1)] = dict((k.strip(), int(v)) for k, v in re.findall(r"remark:\s+([\w /\[\]]+?): (\d+) \[", block))
    text = asm.read_text()
    assert ".amdgcn_target" in text and "gfx950" in text
    bodies, descriptors = {}, {}
    for m in re.finditer(r"^(_ZN12_GLOBAL__N_1\d+(rt_order_[a-z]+_kernel)E\w*):.*?\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        bodies[m.group(2)], descriptors[m.group(2)] = m.group(3), m.group(4)
    return remarks, bodies, descriptors


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
