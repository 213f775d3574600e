"""The kernels of camera views (csrc/rt_view.hip) checked on the CPU: hipcc cross-compiles gfx950 here, with the Makefile's
flags (make asm-view).  Both kernels exist, use no scratch and spill nothing; their float results come from single
multiplies, adds and correctly rounded divisions, never from a fused or packed form the source does not name; and no loop
ends on a per-lane condition."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ("rt_view_rays_kernel", "rt_view_resolve_kernel")
# float forms that fuse or pack (v_mad_u64_u32 and its kin are address arithmetic: only float forms count)
FUSED = r"\b(v_(?:fma|fmac|mad|mac|madak|madmk|fmaak|fmamk|dot\d)_(?:legacy_)?f\d+\w*|v_pk_\w+)"


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """(resource remarks per kernel, assembly body per kernel, kernel descriptor per kernel)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("view_asm") / "rt_view.s"
    r = subprocess.run(["make", "-C", CSRC, "asm-view", "VIEW_ASM_OUT=" + str(asm)], check=True, capture_output=True, text=True, timeout=900)
    remarks = {}
    for block in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(rt_view_[a-z]+_kernel)E", block)
        if m:
            remarks[m.group(1)] = dict((k.strip(), int(v)) for k, v in re.findall(r"remark:\s+([\w /\[\]]+?): (\d+) \[", block))
    text = asm.read_text()
    assert ".amdgcn_target" in text and "gfx950" in text
    bodies, descriptors = {}, {}
    for m in re.finditer(r"^(_ZN12_GLOBAL__N_1\d+(rt_view_[a-z]+_kernel)E\w*):.*?\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        bodies[m.group(2)], descriptors[m.group(2)] = m.group(3), m.group(4)
    return remarks, bodies, descriptors


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


def division_steps(lines, fmas_at):
    """The instructions that compute the quotient a v_div_fmas_f32 at line `fmas_at` finishes: its operands' definitions
    followed backwards, register by register, up to and including the v_div_scale_f32 that start the sequence (what those
    read -- numerator and denominator -- is not part of the division).  -> sorted line numbers"""
    regs = lambda ln: re.findall(r"\bv\d+\b", ln.split(None, 1)[1]) if " " in ln else []  # noqa: E731
    steps, todo = set(), [(fmas_at, r) for r in regs(lines[fmas_at])[1:]]
    while todo:
        before, reg = todo.pop()
        at = next((k for k in range(before - 1, -1, -1) if lines[k].startswith("v_") and regs(lines[k])[:1] == [reg]), None)
        assert at is not None, (lines[before], reg)
        if at in steps:
            continue
        steps.add(at)
        if not lines[at].startswith("v_div_scale_f32"):
            # (v_fmac and v_div_fmas accumulate into their destination: it is an operand too)
            srcs = regs(lines[at]) if lines[at].startswith("v_fmac") else regs(lines[at])[1:]
            todo.extend((at, r) for r in srcs)
    return sorted(steps)


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


def loops_and_exits(body):
    """The control-flow graph of a kernel's assembly -- blocks end at labels and behind branches -- and its loops: the sets of
    blocks that reach one another.  -> [(blocks of the loop, the conditional branches that can leave it)]"""
    blocks, cur = [], {"label": None, "ops": []}
    for ln in body.splitlines():
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1), "ops": []}
            continue
        m = re.match(r"^\s*(s_cbranch_\w+|s_branch|s_endpgm)\b\s*(\.LBB\d+_\d+)?", ln)
        if m:
            cur["ops"].append((m.group(1), m.group(2)))
            blocks.append(cur)
            cur = {"label": None, "ops": []}
    blocks.append(cur)
    index = {b["label"]: i for i, b in enumerate(blocks) if b["label"]}
    succ = []
    for i, b in enumerate(blocks):
        last = b["ops"][-1] if b["ops"] else (None, None)
        out = set()
        if last[0] not in ("s_branch", "s_endpgm") and i + 1 < len(blocks):
            out.add(i + 1)
        if last[1]:
            out.add(index[last[1]])
        succ.append(out)

    def reach(i):
        seen, todo = set(), list(succ[i])
        while todo:
            j = todo.pop()
            if j not in seen:
                seen.add(j)
                todo.extend(succ[j])
        return seen

    reached = [reach(i) for i in range(len(blocks))]
    loops, done = [], set()
    for i in range(len(blocks)):
        if i in done or i not in reached[i]:
            continue
        members = {j for j in reached[i] if i in reached[j]}
        done |= members
        exits = [blocks[j]["ops"][-1][0] for j in members if blocks[j]["ops"] and blocks[j]["ops"][-1][0].startswith("s_cbranch") and
                 not succ[j] <= members]
        loops.append((members, exits))
    return loops


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
