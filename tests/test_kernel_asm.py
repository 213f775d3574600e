"""tests/kernel_asm.py itself, on a few lines of hand-written assembly and remark text (CPU only, no compiler needed but for
the last test)."""
import kernel_asm
from kernel_asm import basic_blocks, divergent_loops, kernel_name, loops_and_exits, parse

ANON = "_ZN12_GLOBAL__N_114rt_rays_kernelE10RtDevScene11RtDevParams9RtRayArgs"
PLAIN = "_Z19rt_lbvh_keys_kernel10RtDevScenePKcPKjPKfPj"
POINTERS = "_ZN12_GLOBAL__N_123rt_selftest_math_kernelEPKfPfS2_j"

LOOP = """\
; %bb.0:
\ts_load_dword s4, s[0:1], 0x0
\ts_cmp_eq_u32 s4, 0
\ts_cbranch_scc1 .LBB0_3
; %bb.1:
\tv_mov_b32_e32 v1, 0
.LBB0_2:                                ; =>This Inner Loop Header: Depth=1
\tv_add_f32_e32 v1, v1, v0
\ts_add_i32 s4, s4, -1
\ts_cmp_lg_u32 s4, 0
\ts_cbranch_scc1 .LBB0_2
.LBB0_3:
\ts_endpgm
"""
STRAIGHT = """\
; %bb.0:
\tv_mul_f32_e32 v0, v0, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB1_2
; %bb.1:
\tglobal_store_dword v1, v0, s[0:1]
.LBB1_2:
\ts_endpgm
"""
DIVERGENT = """\
; %bb.0:
\ts_mov_b64 s[2:3], 0
.LBB2_1:
\tv_cmp_eq_u32_e32 vcc, 0, v0
\ts_or_b64 s[2:3], vcc, s[2:3]
\ts_andn2_b64 exec, exec, s[2:3]
\ts_cbranch_execnz .LBB2_1
; %bb.2:
\ts_endpgm
"""


def function(symbol, body, scratch):
    return (f"\t.globl\t{symbol}\n\t.type\t{symbol},@function\n{symbol}:    ; @{symbol}\n{body}"
            f"\t.section\t.rodata,\"a\",@progbits\n\t.p2align\t6, 0x0\n\t.amdhsa_kernel {symbol}\n"
            f"\t\t.amdhsa_private_segment_fixed_size {scratch}\n\t\t.amdhsa_next_free_vgpr 2\n\t.end_amdhsa_kernel\n\t.text\n")


def remark(symbol, vgprs):
    return (f"x.hip:1:1: remark: Function Name: {symbol} [-Rpass-analysis=kernel-resource-usage]\n"
            f"x.hip:1:1: remark:     VGPRs: {vgprs} [-Rpass-analysis=kernel-resource-usage]\n"
            f"x.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            f"x.hip:1:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]\n")


def test_kernel_name_is_read_by_its_length_prefix():
    assert kernel_name(ANON) == "rt_rays_kernel"          # ...kernelE10RtDevScene: the E closes the namespace, not the name
    assert kernel_name(PLAIN) == "rt_lbvh_keys_kernel"    # no namespace, no E at all
    assert kernel_name(POINTERS) == "rt_selftest_math_kernel"  # ...EPKfPfS2_j
    # a name that itself holds what a search for `E` would stop at
    assert kernel_name("_ZN12_GLOBAL__N_115rt_sEt_E_kernelEPKfPfS2_j") == "rt_sEt_E_kernel"
    assert kernel_name("_Z13rt_sEE_kernelPK6RtNodejPy") == "rt_sEE_kernel"
    assert kernel_name("__hip_cuid_1234") is None and kernel_name("_Z99short") is None


def test_bodies_descriptors_and_remarks_pair_with_their_kernel():
    text = "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + function(ANON, LOOP, 0) + function(PLAIN, STRAIGHT, 16)
    helper = "_ZN12_GLOBAL__N_16helperEf"  # a function that is no kernel: no descriptor, so no entry
    c = parse(text, remark(ANON, 7) + remark(helper, 3) + remark(PLAIN, 9))
    assert set(c.bodies) == set(c.descriptors) == set(c.symbols) == set(c.remarks) == {"rt_rays_kernel", "rt_lbvh_keys_kernel"}
    assert c.symbols["rt_rays_kernel"] == ANON and c.symbols["rt_lbvh_keys_kernel"] == PLAIN
    assert "v_add_f32_e32" in c.bodies["rt_rays_kernel"] and "global_store_dword" not in c.bodies["rt_rays_kernel"]
    assert "global_store_dword" in c.bodies["rt_lbvh_keys_kernel"] and "v_add_f32_e32" not in c.bodies["rt_lbvh_keys_kernel"]
    for name in c.bodies:
        assert c.bodies[name].count("s_endpgm") == 1 and ".amdhsa_" not in c.bodies[name] and "@" + c.symbols[name] not in c.bodies[name]
    assert ".amdhsa_private_segment_fixed_size 0\n" in c.descriptors["rt_rays_kernel"]
    assert ".amdhsa_private_segment_fixed_size 16\n" in c.descriptors["rt_lbvh_keys_kernel"]
    assert c.remarks["rt_rays_kernel"] == {"VGPRs": 7, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 8}
    assert c.remarks["rt_lbvh_keys_kernel"]["VGPRs"] == 9
    assert c.text == text


def test_loops_and_exits():
    loops = loops_and_exits(LOOP)
    assert len(loops) == 1
    members, exits = loops[0]
    assert len(members) == 1 and exits == ["s_cbranch_scc1"]
    assert loops_and_exits(STRAIGHT) == []
    (members, exits), = loops_and_exits(DIVERGENT)
    assert exits == ["s_cbranch_execnz"]


def test_divergent_loops_and_basic_blocks():
    assert [divergent_loops(b) for b in (LOOP, STRAIGHT, DIVERGENT)] == [0, 0, 1]
    assert divergent_loops(DIVERGENT + DIVERGENT) == 2
    # what stands before the first marker, then one piece per `; %bb.N:` and per label
    assert [len(basic_blocks(b)) for b in (LOOP, STRAIGHT, DIVERGENT)] == [1 + 4, 1 + 3, 1 + 3]
    blocks = basic_blocks(LOOP)
    assert blocks[0] == "" and "v_add_f32_e32" in blocks[3] and "v_add_f32_e32" not in blocks[2] and "Inner Loop" not in blocks[3]


def test_a_unit_is_compiled_once_per_process():
    first = kernel_asm.compiled("rt_view")  # (skips without hipcc)
    assert kernel_asm.compiled("rt_view") is first
    assert set(first.bodies) == set(first.descriptors) == set(first.remarks) == {"rt_view_rays_kernel", "rt_view_resolve_kernel"}
