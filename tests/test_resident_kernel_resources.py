"""What hipcc reports about the kernels of the resident walk step (phasm_amd/csrc/resident.hip.h), through the one compile of
tests/resource_utils.py: the family is exact and closed, none spills to scratch, none holds static LDS, and every one stays
within 64 VGPRs (8 waves per SIMD): they stream words or gather by read id, and only resident waves hide the latency of
their loads -- like the walk's own kernels."""
import resource_utils

KERNELS = ("k_rs_flag", "k_rs_local", "k_rs_alnb", "k_rs_paths", "k_rs_commit", "k_rs_or", "k_rs_unmap", "k_rs_popc")
WHY = "these kernels stream words or gather and scatter by read id and are bound by the latency of loads, which only resident waves hide"


def test_no_kernel_of_the_resident_step_spills_or_leaves_its_budget():
    usage = resource_utils.kernel_usage()
    resource_utils.check_kernels(usage, {"exact": True, "family": "k_rs_", "why": WHY,
                                         "forbid": ("k_wk_", "k_rr_", "k_ph_", "k_pp_", "k_spell_"),
                                         "kernels": {k: (64, "8 waves per SIMD") for k in KERNELS},
                                         "lds": {k: 0 for k in KERNELS}})
    # a new kernel of the stage cannot stay outside the guard
    mine = sorted(k for k in usage if "k_rs_" in k)
    assert len(mine) == len(KERNELS), mine
    assert all(usage[k]["ScratchSize"] == 0 and usage[k]["LDS"] == 0 for k in mine)
