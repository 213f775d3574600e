"""Register budget of the config 1-3 render kernel (CPU only: hipcc cross-compiles gfx950 here).

rt_primary_kernel runs at 6 waves per SIMD (80 VGPRs).  Every value it holds through the light loop competes for those
registers, and what does not fit goes to scratch (HBM write-back) or, for SGPRs, into lanes of a VGPR that are read back
with one v_readlane per value.  The kernel arguments are re-read from the kernarg segment where the loops use them
(kernarg_fresh in rt_kernels.hip), and the view direction waits in the LDS stash; this test holds the resulting budget, so
that a change that adds pressure to the light loop fails here, at build time, rather than as a slower frame on the GPU."""
from kernel_asm import compiled

# kernel -> (occupancy in waves per SIMD, SGPR spills, VGPR spills, scratch bytes per lane: each at most).
# Before this budget existed: 6 / 169 / 49 / 108.  The SGPRs still spilled sit in lanes 0-16 of one VGPR (v79); by where
# they are written and read back (make asm, rt_kernels.s; the remark counts 20):
#   * lanes 0-8 and 12: written before the light loop, read after it -- per-wavefront masks and scalars of the pixel
#     mapping and the statistics (once per wavefront each way);
#   * lanes 9-11: the wavefront's first hit point p_first, written once, read once per light by the sphere pre-selection
#     (three v_readlane per light: what taking it from the lanes again would cost as well);
#   * lanes 13-16 (and 0-1 in the backface-culling instantiation): 64-bit lane masks of the candidate classification,
#     spilled and reloaded inside one light iteration.
# None is written or read inside the sample or candidate loops.
BUDGET = {
    "rt_primary_kernel": (6, 20, 14, 28),
}
# the kernels that share process_ray (and its LDS stash) must keep their occupancy
OCCUPANCY = {"rt_primary_stream_kernel": 6, "rt_primary_pre_kernel": 6, "rt_shade_kernel": 6}


def test_primary_kernel_register_budget():
    # make asm: the same flags as the library, plus -Rpass-analysis=kernel-resource-usage (the remarks go to stderr)
    res = compiled("rt_kernels").remarks
    for name, (occ, sgpr_spill, vgpr_spill, scratch) in BUDGET.items():
        assert name in res, (name, sorted(res))
        f = res[name]
        assert f["Occupancy [waves/SIMD]"] == occ, (name, f)
        assert f["SGPRs Spill"] <= sgpr_spill, (name, f)
        assert f["VGPRs Spill"] <= vgpr_spill, (name, f)
        assert f["ScratchSize [bytes/lane]"] <= scratch, (name, f)
    for name, occ in OCCUPANCY.items():
        assert res[name]["Occupancy [waves/SIMD]"] == occ, (name, res[name])
