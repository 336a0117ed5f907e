"""The kernels of po_phase_index and po_phase_relevant (phasm_amd/csrc/relevant.hip.h) stay in registers: no scratch, at most
64 VGPRs -- each holds a handful of indices, one 16-byte entry and a key; nothing is unrolled over data -- and static LDS
within a workgroup's 64 KB (they use none).  The family is counted: a new k_rr_ kernel cannot stay outside the guard, and none
of them carries the prefix of another stage's family."""
import resource_utils

WHY = "one thread or one wave per item: a few indices, one entry {b, a0, a1, seq}, one 64-bit key"
KERNELS = ("k_rr_insert", "k_rr_degree", "k_rr_fill", "k_rr_sort", "k_rr_place", "k_rr_mark", "k_rr_mark_seg", "k_rr_count", "k_rr_select",
           "k_rr_list", "k_rr_alncount", "k_rr_alnwrite", "k_rr_omax")
SPEC = {"kernels": {name: (64, WHY) for name in KERNELS}, "exact": True, "family": "k_rr_",
        "forbid": ("k_ph_", "k_cov_", "k_ct_", "k_bc_", "k_sb_", "k_scc_", "k_cc_", "k_merge_", "k_diamond_", "k_tips_", "k_reduce_"),
        "lds": dict.fromkeys(KERNELS, 64 * 1024), "why": WHY}


def test_relevant_kernels_stay_in_registers():
    resource_utils.check_kernels(resource_utils.kernel_usage(), SPEC)
