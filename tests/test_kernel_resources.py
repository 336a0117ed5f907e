"""Compile-time guard on the kernels' register, scratch and LDS budgets (hipcc cross-compiles gfx950 without a GPU).

A harmless-looking edit to a helper that the scan kernels inline (a different canonical-pair rule) once
took k_scan_fill from 54 to 121 VGPRs and k_scan_probe into scratch, costing 8 % of the step before any
test noticed: parity tests cannot see that, this one can.

The library is one translation unit, so one compile reports every kernel (resource_utils.kernel_usage, once per test
process); STAGES holds what each device stage promises, and resource_utils.check_kernels holds the assertions.  A new stage
adds an entry here, not a file."""
import os
import shutil
import subprocess

import pytest

import resource_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  The graph stages are bound by the latency of dependent gathers,
# which only resident waves hide; each entry's "why" names the gathers (it is printed when a kernel goes over).
WAVES_8 = (64, "8 waves per SIMD")


def each(names, budget=WAVES_8):
    return dict.fromkeys(names, budget)


# The match rule.  The kernels of the graph and phase stages are plain functions of namespace po: "exact" finds \d<name>E
# in the mangled name exactly once, so k_x cannot stand in for k_x_wide.  The hot kernels are templates, listed by the
# prefix of the instantiations that ship (k_scan_probeILi2ELb1...), and every instantiation with the prefix is held.
# "family" counts: the remarks hold exactly the listed kernels with that prefix.  "forbid": a family whose prefix could be
# read into another one's (k_scc_ / k_cc_) shows that no kernel is counted by two entries.
STAGES = {
    # kernel (mangled-name fragment) -> (max VGPRs, why)
    "hot": {
        "exact": False,
        "kernels": {
            "k_scan_probeILi2ELb1": (128, "16 waves per CU: one persistent 1024-thread workgroup"),
            "k_scan_probeILi2ELb0": (128, "same"),
            "k_scan_fillILi2": (64, "8 waves per SIMD"),
            "k_verify_aILi2ELb": (64, "8 waves per SIMD; LDS-limited beyond that"),
            "k_scan_fixupILi2": (64, ""),
            "k_wide_scanILi2ELb0": (64, ""),
            "k_wide_scanILi2ELb1": (64, ""),
            "k_emit": (64, ""),
            "k_layout_classify": (64, ""),
            "k_layout_insert": (64, ""),
            "k_layout_winner": (64, ""),
        },
    },
    "reduce": {    # po_layout_reduce (phasm_amd/csrc/reduce.hip.h)
        "exact": True, "family": "k_reduce_",
        "why": "every kernel here is bound by the latency of dependent gathers (an edge, then its node's lists), which only "
               "resident waves hide.  k_reduce_mark runs one 64-lane workgroup per node with 5 KB of LDS: 32 of them fit a "
               "CU's 160 KB, so registers, not LDS, must not be what limits its occupancy either.",
        "kernels": {
            "k_reduce_degree": (64, "8 waves per SIMD"),
            "k_reduce_maxdeg": (64, "same"),
            "k_reduce_scatter": (64, "same"),
            "k_reduce_order": (64, "same"),
            "k_reduce_mark": (64, "same; LDS allows 32 workgroups of one wave per CU"),
            "k_reduce_symmetric": (64, "same"),
            "k_reduce_emit": (64, "same"),
        },
        "lds": {"k_reduce_mark": 160 * 1024 // 32},
    },
    "tips": {      # po_layout_tips (phasm_amd/csrc/tips.hip.h) and the two node-order kernels of po_layout_edges
        "exact": True, "family": "k_tips_",
        "why": "every kernel here is bound by the latency of dependent gathers (a node's degree, its one edge, the next "
               "node), which only resident waves hide.",
        "kernels": each(("k_tips_degree", "k_tips_candidates", "k_tips_mark", "k_tips_resolve", "k_tips_insert",
                         "k_tips_symmetric", "k_tips_alive", "k_tips_nodes", "k_layout_first_contained", "k_layout_node_rank")),
    },
    "diamond": {   # po_layout_diamonds (phasm_amd/csrc/diamond.hip.h)
        "exact": True, "family": "k_diamond_",
        "why": "every kernel here is bound by the latency of dependent gathers (an end node's in-edges, their sources, those "
               "nodes' in-edges), which only resident waves hide.",
        "kernels": each(("k_diamond_degree", "k_diamond_candidates", "k_diamond_mark", "k_diamond_resolve", "k_diamond_nodes")),
    },
    "merge": {     # po_layout_merge (phasm_amd/csrc/merge.hip.h)
        "exact": True, "family": "k_merge_",
        "why": "every kernel here is bound by the latency of dependent gathers (a node's one edge, that edge's other end, "
               "that node's degree; jb[jb[n]] in a round), which only resident waves hide.",
        "kernels": each(("k_merge_degree", "k_merge_links", "k_merge_jump", "k_merge_tails", "k_merge_bitonic", "k_merge_number",
                         "k_merge_tables", "k_merge_ranks", "k_merge_edges")),
    },
    "coverage": {  # po_layout_coverage (phasm_amd/csrc/coverage.hip.h)
        "exact": True, "family": "k_cov_",
        "why": "every kernel here is bound by the latency of dependent gathers, which only resident waves hide: a row's read, "
               "that read's node, the probe sequence of the pair table (k_cov_insert); a slot's node, that node's offset "
               "(k_cov_fill); an edge's two nodes, their lists, each entry's probe sequence and that read's length "
               "(k_cov_edges); the binary search of k_cov_members.  k_cov_mark, _nodes and _max stream and need few.",
        "kernels": each(("k_cov_mark", "k_cov_nodes", "k_cov_members", "k_cov_insert", "k_cov_max", "k_cov_fill", "k_cov_edges")),
    },
    "components": {  # po_layout_components (phasm_amd/csrc/components.hip.h)
        "exact": True, "family": "k_cc_",
        "why": "these kernels stream or gather and are bound by the latency of dependent loads, which only resident waves "
               "hide: an edge's two ranks and their parent words (k_cc_hook), a rank's parent and grandparent (k_cc_jump), a "
               "rank's root and that root's index (k_cc_label_nodes).",
        "kernels": each(("k_cc_keys", "k_cc_init", "k_cc_ends", "k_cc_hook", "k_cc_jump", "k_cc_roots", "k_cc_label_nodes",
                         "k_cc_label_edges", "k_cc_max")),
    },
    "partition": {  # po_layout_partition (phasm_amd/csrc/partition.hip.h)
        "exact": True, "family": "k_scc_", "forbid": ("k_cc_",),
        "why": "these kernels stream or gather and are bound by the latency of dependent loads, which only resident waves "
               "hide: an edge's two ranks, their live bytes and their colour words or mark bytes (k_scc_trim_edges, "
               "k_scc_forward, k_scc_backward), an edge's two SCCs and their table entries (k_scc_edges), a rank's root and "
               "that root's index (k_scc_label_nodes).",
        "kernels": each(("k_scc_init", "k_scc_trim_edges", "k_scc_trim_ranks", "k_scc_colour_init", "k_scc_forward",
                         "k_scc_back_init", "k_scc_backward", "k_scc_retire", "k_scc_roots", "k_scc_label_nodes", "k_scc_edges",
                         "k_scc_flags", "k_scc_max")),
    },
    "superbubbles": {  # po_layout_superbubbles (phasm_amd/csrc/superbubbles.hip.h)
        "exact": True, "family": "k_sb_", "forbid": ("k_scc_", "k_cc_"),
        "why": "these kernels stream or gather and are bound by the latency of dependent loads, which only resident waves "
               "hide: an edge's two ranks and their level words (k_sb_level), a rank's list and, per neighbour, the two "
               "chains of the tree (k_sb_tree), a rank's dominator and that one's exit (k_sb_encl, k_sb_label).",
        "kernels": each(("k_sb_init", "k_sb_degrees", "k_sb_fill", "k_sb_nodes", "k_sb_level", "k_sb_level_max", "k_sb_tree",
                         "k_sb_pairs", "k_sb_encl", "k_sb_dead_init", "k_sb_dead_round", "k_sb_label", "k_sb_sum", "k_sb_table")),
    },
    "bubblechains": {  # po_layout_bubblechains (phasm_amd/csrc/bubblechains.hip.h)
        "exact": True, "family": "k_bc_", "forbid": ("k_sb_", "k_scc_", "k_cc_"),
        "why": "these kernels gather and are bound by the latency of dependent loads, which only resident waves hide: a rank's "
               "pointer and that one's pointer (k_bc_nest, k_bc_jump), a rank's holder, its head and the head's flag word "
               "(k_bc_place), an edge's two ranks and their heads (k_bc_edges, k_bc_edge_out).",
        "kernels": each(("k_bc_init", "k_bc_link", "k_bc_heads", "k_bc_nest", "k_bc_jump", "k_bc_place", "k_bc_edges",
                         "k_bc_filter", "k_bc_table", "k_bc_nodes", "k_bc_edge_out")),
    },
    "contigs": {   # po_layout_contigs (phasm_amd/csrc/contigs.hip.h)
        "exact": True, "family": "k_ct_", "forbid": ("k_sb_", "k_scc_", "k_cc_", "k_bc_"),
        "why": "these kernels gather and are bound by the latency of dependent loads, which only resident waves hide: an edge's "
               "link and that one's link (k_ct_jump, k_ct_cover_jump), an edge's first rank, its in-edge and that one's class "
               "(k_ct_links, k_ct_cover_init), an edge's head and the head's words (k_ct_paths, k_ct_edge_out).",
        "kernels": each(("k_ct_init", "k_ct_degrees", "k_ct_classes", "k_ct_links", "k_ct_jump", "k_ct_cover_init",
                         "k_ct_cover_jump", "k_ct_paths", "k_ct_filter", "k_ct_isolated", "k_ct_keys", "k_ct_number",
                         "k_ct_iso_table", "k_ct_edge_out")),
    },
    "phase": {     # po_phase_branch (phasm_amd/csrc/phase.hip.h): no scratch, and the static LDS fits a workgroup's 64 KB
        "exact": True, "family": "k_ph_",
        "kernels": each(("k_ph_bits", "k_ph_intervals", "k_ph_table", "k_ph_extend", "k_ph_gather", "k_ph_levels",
                         "k_ph_survive"), (None, "")),
    },
    "relevant": {  # po_phase_index and po_phase_relevant (phasm_amd/csrc/relevant.hip.h): no scratch, at most 64 VGPRs --
        # nothing is unrolled over data -- and static LDS within a workgroup's 64 KB (they use none)
        "exact": True, "family": "k_rr_",
        "forbid": ("k_ph_", "k_cov_", "k_ct_", "k_bc_", "k_sb_", "k_scc_", "k_cc_", "k_merge_", "k_diamond_", "k_tips_", "k_reduce_"),
        "why": "one thread or one wave per item: a few indices, one entry {b, a0, a1, seq}, one 64-bit key",
        "kernels": each(("k_rr_insert", "k_rr_degree", "k_rr_fill", "k_rr_sort", "k_rr_place", "k_rr_mark", "k_rr_mark_seg",
                         "k_rr_count", "k_rr_select", "k_rr_list", "k_rr_alncount", "k_rr_alnwrite", "k_rr_omax"),
                        (64, "one thread or one wave per item: a few indices, one entry {b, a0, a1, seq}, one 64-bit key")),
    },
    "spell": {     # po_spell (phasm_amd/csrc/spell.hip.h)
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
    },
}
for _stage in ("phase", "relevant"):
    STAGES[_stage]["lds"] = dict.fromkeys(STAGES[_stage]["kernels"], 64 * 1024)


def test_hot_kernels_stay_in_registers():
    usage = resource_utils.kernel_usage()
    assert len(usage) > 20
    resource_utils.check_kernels(usage, STAGES["hot"])
    # nothing in the library may spill
    spills = {k: v["ScratchSize"] for k, v in usage.items() if v.get("ScratchSize")}
    assert not spills, spills


@pytest.mark.parametrize("stage", [s for s in STAGES if s != "hot"], ids=str)
def test_stage_kernels_stay_within_their_budget(stage):
    resource_utils.check_kernels(resource_utils.kernel_usage(), STAGES[stage])


def test_the_resource_guard_fails_when_it_should():
    """check_kernels on made-up remarks, without a compile: every kind of fault it is there for must raise, so that an edit of
    the shared checker cannot quietly turn all the guards above into none."""
    ok = {"VGPRs": 40, "ScratchSize": 0, "LDS": 512}
    clean = {"_ZN2po7k_x_oneEPj": dict(ok), "_ZN2po7k_x_twoEPKjPj": dict(ok), "_ZN2po7k_y_oneEPj": dict(ok)}
    spec = {"exact": True, "family": "k_x_", "forbid": ("k_y_",), "lds": {"k_x_two": 1024},
            "kernels": {"k_x_one": (64, "8 waves per SIMD"), "k_x_two": (64, "same")}}
    resource_utils.check_kernels(clean, spec)
    resource_utils.check_kernels(clean, dict(spec, exact=False))

    def changed(name=None, drop=None, **fields):
        usage = {k: dict(v) for k, v in clean.items() if k != drop}
        if name:
            usage.setdefault(name, dict(ok)).update(fields)
        return usage
    faults = {   # what is wrong: (the remarks, what the message must say)
        "a listed kernel is missing": (changed(drop="_ZN2po7k_x_twoEPKjPj"), "kernel k_x_two not found"),
        "over the VGPR budget": (changed("_ZN2po7k_x_oneEPj", VGPRs=65), r"k_x_oneEPj uses 65 VGPRs \(budget 64"),
        "scratch": (changed("_ZN2po7k_x_twoEPKjPj", ScratchSize=8), "k_x_twoEPKjPj spills to scratch"),
        "over the LDS limit": (changed("_ZN2po7k_x_twoEPKjPj", LDS=1025), "k_x_twoEPKjPj holds 1025 bytes of static LDS"),
        "one kernel more in the family than on the list": (changed("_ZN2po9k_x_threeEPj"), "not on the list: .*k_x_threeEPj"),
        "a family member of a forbidden family too": (changed("_ZN2po7k_x_oneEPNS_5k_y_tE", drop="_ZN2po7k_x_oneEPj"),
                                                      r"the k_y_\* list counts too: .*k_x_oneEPNS_5k_y_tE"),
    }
    for usage, message in faults.values():
        for exact in (True, False):
            with pytest.raises(AssertionError, match=message):
                resource_utils.check_kernels(usage, dict(spec, exact=exact))
    with pytest.raises(AssertionError, match="kernel k_x_one not found once"):   # a name that matches twice, exact rule only
        resource_utils.check_kernels(changed("_ZN2po5inner7k_x_oneEPj"), spec)


def test_the_remarks_are_read_in_full():
    """All three figures of every kernel, from the compiler's text as it stands in a build log."""
    text = ("c_api.hip:9:1: remark: Function Name: _ZN2po7k_x_oneEPj [-Rpass-analysis=kernel-resource-usage]\n"
            "c_api.hip:9:1: remark:     VGPRs: 12 [-Rpass-analysis=kernel-resource-usage]\n"
            "c_api.hip:9:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "c_api.hip:9:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "c_api.hip:9:1: remark:     LDS Size [bytes/block]: 5120 [-Rpass-analysis=kernel-resource-usage]\n")
    assert resource_utils.parse_remarks(text) == {"_ZN2po7k_x_oneEPj": {"VGPRs": 12, "ScratchSize": 0, "LDS": 5120}}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_scan_pipeline_never_reads_a_register_whose_load_is_in_flight():
    """k_scan_probe issues its steady-state loads with inline asm and waits for them with counted s_waitcnt
    statements; hipcc does not know those registers are pending.  Two asm waits in the arms of an `if` once made
    it copy the landing registers in FRONT of the wait (stale data, and the parity tests still passed on that
    build): tools/check_scan_isa.py walks the generated code for exactly that."""
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scan_isa.py"), "--strict"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert "0 problem(s)" in out.stdout


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_isa_walk_was_validated_for_this_compiler():
    """The walk above is only as good as its reading of the compiler's output.  A hipcc whose code for k_scan_probe nobody
    has looked at is a FAILURE of its own, by name and with instructions (the hand-scheduled scan relies on the compiler
    leaving the landing registers of in-flight loads alone: a new compiler must not ship a library unseen)."""
    from phasm_amd import build
    v = build.hipcc_version(shutil.which("hipcc"))
    assert v in build.VALIDATED_HIPCC, (
        "hipcc %s: look at k_scan_probe's generated code again (tools/check_scan_isa.py), then add the version to "
        "phasm_amd/build.py:VALIDATED_HIPCC" % v)
