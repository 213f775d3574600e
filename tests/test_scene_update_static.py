"""The kernels of in-place scene updates (csrc/rt_update.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the
Makefile's flags (make asm-update).  Every kernel exists and uses no scratch; the kernels that write records out of single
multiplies and adds contain no fused or packed multiply-add, so their results are the host model's bit for bit; and the
new sources keep to vector stores."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ("rt_upd_spheres_kernel", "rt_upd_slots_kernel", "rt_upd_tris_kernel", "rt_upd_nodes_kernel", "rt_upd_octants_kernel",
           "rt_upd_threaded_kernel", "rt_upd_bounds_kernel", "rt_upd_recv_kernel", "rt_upd_materials_kernel", "rt_upd_lights_kernel")
# Float results here come from single multiplies and adds only.  (The others divide or take square roots -- sphere radius
# bounds, scene bounds, material constants, fp64 receiver maps -- and the compiler's correctly rounded division and sqrt
# sequences are built from fused steps; their sources use the same single operations around them.)
RECORD_KERNELS = ("rt_upd_slots_kernel", "rt_upd_tris_kernel", "rt_upd_nodes_kernel", "rt_upd_octants_kernel", "rt_upd_threaded_kernel",
                  "rt_upd_lights_kernel")
NEW_SOURCES = ("rt_update.hip", "rt_update.cpp", "rt_refit.h")


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("update_asm") / "rt_update.s"
    r = subprocess.run(["make", "-C", CSRC, "asm-update", "UPDATE_ASM_OUT=" + str(asm)], check=True, capture_output=True, text=True, timeout=900)
    remarks = {}
    for block in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_Z\d+(rt_upd_[a-z]+_kernel)", block)
        if m:
            remarks[m.group(1)] = dict((k.strip(), int(v)) for k, v in re.findall(r"remark:\s+([\w /\[\]]+?): (\d+) \[", block))
    text = asm.read_text()
    bodies, descriptors = {}, {}
    for m in re.finditer(r"^(_Z\d+(rt_upd_[a-z]+_kernel)\w*):.*?\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        bodies[m.group(2)], descriptors[m.group(2)] = m.group(3), m.group(4)
    return remarks, bodies, descriptors


def test_every_update_kernel_is_built(build):
    remarks, bodies, descriptors = build
    for name in KERNELS:
        assert name in remarks and name in bodies and name in descriptors, (name, sorted(bodies))
        assert "s_endpgm" in bodies[name]


@pytest.mark.parametrize("name", KERNELS)
def test_update_kernel_uses_no_scratch(build, name):
    remarks, bodies, descriptors = build
    print(name, remarks[name])
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptors[name]), name
    assert remarks[name]["ScratchSize [bytes/lane]"] == 0 and remarks[name]["VGPRs Spill"] == 0 and remarks[name]["SGPRs Spill"] == 0
    assert not re.search(r"\b(scratch_|buffer_)(load|store)", bodies[name]), name


@pytest.mark.parametrize("name", RECORD_KERNELS)
def test_record_kernel_has_no_fused_or_packed_multiply_add(build, name):
    _, bodies, _ = build
    # (v_mad_u64_u32 and its kin are address arithmetic: only float forms count)
    fused = re.findall(r"\b(v_(?:fma|fmac|mad|mac|madak|madmk|fmaak|fmamk|dot\d)_(?:legacy_)?f\d+\w*|v_pk_\w+)", bodies[name])
    assert not fused, (name, sorted(set(fused)))


def test_slots_kernel_multiplies_and_adds_separately(build):
    """X = e1 x e2 of an intersection record: six products, three sums"""
    _, bodies, _ = build
    body = bodies["rt_upd_slots_kernel"]
    assert len(re.findall(r"\bv_mul_f32", body)) == 6 and len(re.findall(r"\bv_(?:sub|add|subrev)_f32", body)) == 3


def test_no_kernel_waits_for_another_workgroup(build):
    """the refit is ordered by launch boundaries alone: no loop of any update kernel sleeps or polls memory"""
    _, bodies, _ = build
    for name in KERNELS:
        assert "s_sleep" not in bodies[name] and not re.search(r"\b(global|flat)_atomic_cmpswap", bodies[name]), name


def test_new_sources_keep_to_vector_stores():
    words = [a + b for a in ("s_", "s_buffer_", "s_scratch_") for b in ("store", "atomic")] + ["s_dcache_" + x for x in ("wb", "discard")]
    for f in NEW_SOURCES:
        src = open(os.path.join(CSRC, f)).read().lower()
        for w in words:
            assert w not in src, (f, w)
        assert "asm(" not in src and "asm volatile" not in src, f
