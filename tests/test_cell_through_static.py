"""The list kernels with the marks of certain glass-pane crossings (csrc/rt_kernels.hip: the list-union block, the list route of
collect_light_candidates and the sample loop of shadow_ray), checked in the assembly hipcc makes for gfx950 (cross-compiled
here, no GPU needed): rt_primary_soft{10,19,28}_kernel keep 6 waves per SIMD, spill and use scratch no more than the generic
kernel does, hold no loop whose exit is decided lane by lane, and really read the marks (a byte load in each of them, which
the flags-only kernels do not have)."""
import re

import pytest

from kernel_asm import compiled, divergent_loops

GENERIC = "rt_primary_kernel"
LIST = tuple(f"rt_primary_soft{n}_kernel" for n in (10, 19, 28))
FLAGS = tuple(f"rt_primary_soft{n}_flags_kernel" for n in (10, 19, 28))
BYTE_LOAD = re.compile(r"\b(?:global|flat)_load_ubyte\b")


@pytest.fixture(scope="module")
def build():
    c = compiled("rt_kernels")
    return c.remarks, c.bodies


@pytest.mark.parametrize("name", LIST)
def test_list_kernels_keep_their_register_budget(build, name):
    remarks, _ = build
    r, g = remarks[name], remarks[GENERIC]
    print(name, {k: r[k] for k in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")})
    assert r["Occupancy [waves/SIMD]"] == 6, r
    for key in ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]"):
        assert r[key] <= g[key], (name, key, r[key], g[key])


@pytest.mark.parametrize("name", LIST)
def test_list_kernels_have_no_divergent_loop(build, name):
    _, bodies = build
    assert divergent_loops(bodies[name]) == 0, name


def test_only_the_list_kernels_read_the_marks(build):
    _, bodies = build
    for name in LIST:
        assert BYTE_LOAD.search(bodies[name]), f"{name} reads a mark byte"
    for name in FLAGS:
        assert not BYTE_LOAD.search(bodies[name]), f"{name} reads no marks"
