"""What hipcc makes of a kernel file for gfx950, for the tests that check kernels on the CPU: compiled(unit) runs the
Makefile's assembly rule once per process and unit and hands out the resource remarks, assembly bodies and kernel
descriptors per kernel; the helpers below read a body.  A new kernel file needs no Makefile target and no fixture of its
own, only compiled("rt_<name>")."""
import functools
import os
import re
import shutil
import subprocess
import tempfile
import types
from dataclasses import dataclass

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hslu_i", "ba_raytracing", "f2501_raytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

UNITS = ("rt_kernels", "rt_update", "rt_order", "rt_view", "rt_view_adapt", "rt_pose", "rt_sah", "rt_rebuild", "rt_ploc", "rt_skin")


@dataclass(frozen=True)
class Compiled:
    remarks: types.MappingProxyType      # kernel -> {field of the resource-usage remark: int}
    bodies: types.MappingProxyType       # kernel -> assembly text between its label and its descriptor
    descriptors: types.MappingProxyType  # kernel -> the lines between .amdhsa_kernel and .end_amdhsa_kernel
    symbols: types.MappingProxyType      # kernel -> mangled symbol
    text: str                            # the whole .s


def kernel_name(symbol):
    """The function's own name, read by its length prefix: _Z[N12_GLOBAL__N_1]<len><name>...  (None: not such a symbol)"""
    m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", symbol)
    if not m:
        return None
    name = symbol[m.end():m.end() + int(m.group(1))]
    return name if len(name) == int(m.group(1)) else None


def parse(text, stderr):
    """-> Compiled, of the text of a .s and the compiler's stderr.  A kernel is what has a descriptor; the remarks of other
    functions are left out."""
    bodies, descriptors, symbols, remarks = {}, {}, {}, {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        name = kernel_name(m.group(1))
        label = re.search(r"^%s:.*\n" % re.escape(m.group(1)), text, re.M)
        if name is None or label is None or label.end() > m.start():
            continue
        assert name not in symbols, (name, symbols[name], m.group(1))
        bodies[name], descriptors[name], symbols[name] = text[label.end():m.start()], m.group(2), m.group(1)
    by_symbol = {s: k for k, s in symbols.items()}
    for block in re.split(r"remark: Function Name: ", stderr)[1:]:
        name = by_symbol.get(block.split(None, 1)[0])
        if name:
            remarks[name] = dict((k.strip(), int(v)) for k, v in re.findall(r"remark:\s+([\w /\[\]]+?): (\d+) \[", block))
    return Compiled(*(types.MappingProxyType(d) for d in (remarks, bodies, descriptors, symbols)), text)


@functools.lru_cache(maxsize=None)
def compiled(unit):
    """make asm UNIT=<unit> into a temporary directory, once per process: every module of a test run reads the same record"""
    assert unit in UNITS, unit
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, unit + ".s")
        r = subprocess.run(["make", "-C", CSRC, "asm", "UNIT=" + unit, "ASM_OUT=" + asm], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"make asm UNIT={unit} failed ({r.returncode}):\n" + r.stderr[-4000:])
        text = open(asm).read()
    assert ".amdgcn_target" in text and "gfx950" in text
    return parse(text, r.stderr)


def build(*units):
    """(remarks, bodies, descriptors) of the units together: the shape the static tests' fixtures hand out"""
    cs = [compiled(u) for u in units]
    return tuple({k: v for c in cs for k, v in getattr(c, part).items()} for part in ("remarks", "bodies", "descriptors"))


# float forms that fuse or pack (v_mad_u64_u32 and its kin are address arithmetic: only float forms count)
FUSED = r"\b(v_(?:fma|fmac|mad|mac|madak|madmk|fmaak|fmamk|dot\d)_(?:legacy_)?f\d+\w*|v_pk_\w+)"


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


def basic_blocks(body):
    """a basic block starts at a label or at a `; %bb.N:` comment"""
    return re.split(r"^(?:\.LBB\d+_\d+:|; %bb\.\d+:).*$", body, flags=re.M)


def divergent_loops(body):
    """a loop that narrows EXEC lane by lane ends in `s_andn2_b64 exec, exec, ...` + `s_cbranch_execnz/z`"""
    return len(re.findall(r"s_andn2_b64 exec, exec,", body))
