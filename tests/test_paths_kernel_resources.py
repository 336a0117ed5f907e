"""What hipcc reports about the kernels of po_phase_paths (phasm_amd/csrc/paths.hip.h), through the one compile of
tests/resource_utils.py: no kernel of the stage spills to scratch -- the count and the walk, whose loops over the successors
are the hot path, least of all -- none holds static LDS beyond the counters' reduction, and every one stays within 64 VGPRs
(8 waves per SIMD): they gather, and only resident waves hide the latency of their dependent loads (a member's segment, the
edge behind a key, its head, the head's count)."""
import resource_utils

PLAIN = ("k_pp_bitonic", "k_pp_chain_counts", "k_pp_bubbles", "k_pp_keys", "k_pp_segments", "k_pp_count", "k_pp_table", "k_pp_bubble_nodes",
         "k_pp_preds", "k_pp_inside_keys", "k_pp_inside")
WALKS = ("k_pp_walkILb0E", "k_pp_walkILb1E")          # the length pass and the writing pass
WHY = "these kernels gather and are bound by the latency of dependent loads, which only resident waves hide"
REDUCTION = 4 * 4 * 8                                 # block_add<4>: four counters of four waves


def test_no_kernel_of_the_stage_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    resource_utils.check_kernels(usage, {"exact": True, "family": None, "why": WHY,
                                         "kernels": {k: (64, "8 waves per SIMD") for k in PLAIN},
                                         "lds": {k: REDUCTION for k in PLAIN}})
    resource_utils.check_kernels(usage, {"exact": False, "family": "k_pp_walk", "why": WHY,
                                         "kernels": {k: (64, "8 waves per SIMD") for k in WALKS},
                                         "lds": {k: REDUCTION for k in WALKS}})
    # a new kernel of the stage cannot stay outside the guard, and no kernel of another stage carries the prefix
    mine = sorted(k for k in usage if "k_pp_" in k)
    assert len(mine) == len(PLAIN) + len(WALKS), mine
    assert all(usage[k]["ScratchSize"] == 0 for k in mine)
    assert not [k for k in mine if any(other in k for other in ("k_bc_", "k_sb_", "k_scc_", "k_cc_", "k_ct_", "k_rr_", "k_ph_", "k_spell_"))]
