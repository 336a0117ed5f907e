"""What hipcc reports about the kernels of the resident walk (phasm_amd/csrc/walk.hip.h), through the one compile of
tests/resource_utils.py: none spills to scratch, none holds static LDS (the greatest log_rl goes through the wave and one
integer atomic, no block reduction), and every one stays within 64 VGPRs (8 waves per SIMD): they stream rows or chase links,
and only resident waves hide the latency of their loads."""
import resource_utils

KERNELS = ("k_wk_advance", "k_wk_trace", "k_wk_max", "k_wk_pick")
WHY = "these kernels stream bit rows or chase the links of a candidate and are bound by the latency of loads, which only resident waves hide"
REDUCTION = 4 * 8                                     # at most one value of each of a workgroup's four waves


def test_no_kernel_of_the_walk_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    resource_utils.check_kernels(usage, {"exact": True, "family": "k_wk_", "why": WHY,
                                         "forbid": ("k_ph_", "k_pp_", "k_rr_", "k_spell_"),
                                         "kernels": {k: (64, "8 waves per SIMD") for k in KERNELS},
                                         "lds": {k: REDUCTION for k in KERNELS}})
    # a new kernel of the stage cannot stay outside the guard
    mine = sorted(k for k in usage if "k_wk_" in k)
    assert len(mine) == len(KERNELS), mine
    assert all(usage[k]["ScratchSize"] == 0 for k in mine)
