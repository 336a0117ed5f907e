"""Compile-time guard on the kernels of po_spell (phasm_amd/csrc/spell.hip.h): the entry of this stage for
resource_utils.check_kernels, on the one compile of the library that the resource guards share."""
import resource_utils

SPELL = {
    "exact": True, "family": "k_spell_",
    "why": "k_spell_decode is bound by the latency of its dependent loads -- the binary search over the piece offsets, then the "
           "read's offset, then its words -- which only resident waves hide; it holds 16 output bytes and a few counters per "
           "lane and needs neither LDS nor scratch.",
    "kernels": {
        "k_spell_offsets": (64, "8 waves per SIMD"),
        "k_spell_decode": (64, "same"),
        "k_spell_patch": (64, "same"),
    },
    "lds": {"k_spell_offsets": 0, "k_spell_decode": 0, "k_spell_patch": 0},
}


def test_spell_kernels_stay_within_their_budget():
    resource_utils.check_kernels(resource_utils.kernel_usage(), SPELL)
