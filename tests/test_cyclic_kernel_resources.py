"""What hipcc reports about the kernels of po_layout_superbubbles_all (phasm_amd/csrc/cyclic.hip.h), through the one compile
of tests/resource_utils.py: none spills to scratch, none holds static LDS beyond the counters' reduction, and every one stays
within 64 VGPRs (8 waves per SIMD): they stream or gather, and only resident waves hide the latency of their dependent loads
(an edge's head, its split byte and its copy's number; a rank's SCC and that one's table entry; a rank's exit and that one's
original rank)."""
import resource_utils

KERNELS = ("k_cy_flat", "k_cy_ranks", "k_cy_choose", "k_cy_apply", "k_cy_level0", "k_cy_uncertain", "k_cy_seed_edges", "k_cy_seed_ranks",
           "k_cy_merge", "k_cy_bfs_init", "k_cy_bfs_round", "k_cy_bfs_parents", "k_cy_loops", "k_cy_final")
WHY = "these kernels stream or gather and are bound by the latency of dependent loads, which only resident waves hide"
REDUCTION = 3 * 4 * 8                                 # block_add<3>: three counters of four waves


def test_no_kernel_of_the_stage_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    resource_utils.check_kernels(usage, {"exact": True, "family": "k_cy_", "why": WHY,
                                         "forbid": ("k_sb_", "k_scc_", "k_cc_", "k_bc_", "k_ct_", "k_pp_"),
                                         "kernels": {k: (64, "8 waves per SIMD") for k in KERNELS},
                                         "lds": {k: REDUCTION for k in KERNELS}})
    # a new kernel of the stage cannot stay outside the guard
    mine = sorted(k for k in usage if "k_cy_" in k)
    assert len(mine) == len(KERNELS), mine
    assert all(usage[k]["ScratchSize"] == 0 for k in mine)
    # the kernels the call shares with its siblings are the siblings' own: nothing of them was copied under another name
    assert sum("k_sb_" in k for k in usage) == 14 and sum("k_scc_" in k for k in usage) == 13
