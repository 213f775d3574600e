"""The memo of the last transmissive shadow occluder (OccMemo, csrc/rt_kernels.hip), checked in the assembly hipcc makes for
gfx950 (cross-compiled here, no GPU needed).

In rt_primary_soft10_kernel the block that adds a transmissive occluder to a shadow ray's sums -- the one with the
saturating `v_min_u32 ..., 0x10000000` (RT_SH_ONE) -- no longer converts the material's absorption to integers: no
v_rndne_f32 and no multiply by 2^24 (0x4b800000, RT_FILT_SCALE) in it.  Those conversions now stand only where the memo is
refilled, next to the v_readfirstlane_b32 that move the results to scalar registers.  rt_primary_kernel, which keeps no
memo, still has them in its accumulate blocks (which also shows that the test can see them).  And the kernels keep their
register budget."""
import re

import pytest

from kernel_asm import basic_blocks, compiled

GENERIC = "rt_primary_kernel"
MEMO = tuple(f"rt_primary_soft{n}_kernel" for n in (10, 19, 28))
SPECIALISED = MEMO + tuple(f"rt_primary_soft{n}_flags_kernel" for n in (10, 19, 28))
# every kernel that holds an instantiation of process_ray
SHARE_PROCESS_RAY = (GENERIC,) + SPECIALISED + ("rt_primary_stream_kernel", "rt_primary_pre_kernel", "rt_shade_kernel", "rt_rays_kernel",
                                                 "rt_rays_stream_kernel")
SATURATE = re.compile(r"v_min_u32_e32 v\d+, 0x10000000, v\d+")
FILT_SCALE = "0x4b800000"


@pytest.fixture(scope="module")
def build():
    """(resource remarks per kernel, basic blocks per kernel)"""
    c = compiled("rt_kernels")
    return c.remarks, {name: basic_blocks(body) for name, body in c.bodies.items()}


def accumulate_blocks(blocks):
    return [b for b in blocks if SATURATE.search(b)]


@pytest.mark.parametrize("name", MEMO)
def test_accumulate_blocks_no_longer_convert_the_absorption(build, name):
    _, blocks = build
    acc = accumulate_blocks(blocks[name])
    # sphere loop and candidate-triangle loop of the list route, the walk route's leaves
    assert len(acc) >= 2, (name, len(acc))
    for b in acc:
        assert "v_rndne_f32" not in b and FILT_SCALE not in b, (name, b)
    # the conversions stand where the memo is refilled, and nowhere else
    refill = [b for b in blocks[name] if FILT_SCALE in b]
    assert refill, name
    for b in refill:
        assert b.count("v_rndne_f32") >= 3 and b.count("v_readfirstlane_b32") >= 3, (name, b)


def test_the_kernel_without_memo_still_converts_per_occluder(build):
    _, blocks = build
    acc = accumulate_blocks(blocks[GENERIC])
    assert acc, GENERIC
    for b in acc:
        assert b.count("v_rndne_f32") >= 4 and FILT_SCALE in b, (GENERIC, b)  # three absorption terms and the opacity decrement


def test_register_budget_is_kept(build):
    remarks, _ = build
    for name in SHARE_PROCESS_RAY:
        assert remarks[name]["Occupancy [waves/SIMD]"] == 6, (name, remarks[name])
    g = remarks[GENERIC]
    assert g["SGPRs Spill"] <= 20 and g["VGPRs Spill"] <= 14 and g["ScratchSize [bytes/lane]"] <= 28, g
    for name in SPECIALISED:
        for key in ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]"):
            assert remarks[name][key] <= g[key], (name, key, remarks[name][key], g[key])
