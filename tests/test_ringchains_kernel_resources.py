"""What hipcc reports about the kernels of the ring election (phasm_amd/csrc/ringchains.hip.h), through the one compile of
tests/resource_utils.py: none spills to scratch, none holds static LDS, and every one stays within 64 VGPRs (8 waves per
SIMD), the budget of the sibling stages for the same reason: they stream or gather, and only resident waves hide the latency
of their dependent loads (a rank's pointer, then that rank's pointer and minimum; a leader's pointer, then that rank's word)."""
import resource_utils

KERNELS = ("k_rc_init", "k_rc_round", "k_rc_leaders", "k_rc_close")
WHY = "these kernels stream or gather and are bound by the latency of dependent loads, which only resident waves hide"
OTHERS = ("k_bc_", "k_sb_", "k_scc_", "k_cy_", "k_ct_", "k_pp_", "k_cc_")


def test_no_kernel_of_the_election_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    resource_utils.check_kernels(usage, {"exact": True, "family": "k_rc_", "why": WHY, "forbid": OTHERS,
                                         "kernels": {k: (64, "8 waves per SIMD") for k in KERNELS},
                                         "lds": {k: 0 for k in KERNELS}})
    # a new kernel of the election cannot stay outside the guard
    mine = sorted(k for k in usage if "k_rc_" in k)
    assert len(mine) == len(KERNELS), mine
    assert all(usage[k]["ScratchSize"] == 0 for k in mine)
    # the kernels around the election are the siblings' own: nothing of them was copied under another name
    assert sum("k_bc_" in k for k in usage) == 11 and sum("k_cy_" in k for k in usage) == 14 and sum("k_sb_" in k for k in usage) == 14
