"""What hipcc reports about the kernels of po_phase_large (phasm_amd/csrc/large.hip.h), through the one compile of
tests/resource_utils.py: the family is listed exactly, none spills to scratch, every one stays within 64 VGPRs, and the static
LDS of k_lg_score -- two tile arrays, one chunk of slots, the wave sums -- stays within a workgroup's 64 KB, in fact within the
20 KB at which eight workgroups share a compute unit's 160 KB."""
import resource_utils

KERNELS = ("k_lg_slots", "k_lg_score", "k_lg_best_key", "k_lg_best_idx")
WHY = ("k_lg_score joins 8-byte intervals that it loads per (slot, read) from a table that sits in the caches: it is bound by the "
       "latency of those loads, which only resident waves hide -- 512 VGPRs per SIMD lane / 64 = the 8 waves per SIMD that "
       "__launch_bounds__(256) with eight workgroups per compute unit asks for; the other three stream one array once")
TILES = 2 * 4 * 2048 + 4 * 256 + 8 * 4                # s_s0 and s_e of PH_TILE reads, LG_CHUNK slots, one double per wave
WORKGROUP = 64 * 1024


def test_no_kernel_of_the_large_arm_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    assert TILES <= 20 * 1024 <= WORKGROUP
    resource_utils.check_kernels(usage, {"exact": True, "family": "k_lg_", "why": WHY,
                                         "forbid": ("k_ph_", "k_pp_", "k_wk_", "k_rr_", "k_spell_"),
                                         "kernels": {k: (64, "8 waves per SIMD") for k in KERNELS},
                                         "lds": {"k_lg_score": TILES, "k_lg_slots": 0, "k_lg_best_key": 0, "k_lg_best_idx": 0}})
    mine = sorted(k for k in usage if "k_lg_" in k)
    assert len(mine) == len(KERNELS), mine
    assert all(usage[k]["ScratchSize"] == 0 and usage[k]["LDS"] <= WORKGROUP for k in mine)
