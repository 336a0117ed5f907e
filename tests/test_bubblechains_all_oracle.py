"""``phasm_amd.cyclic.HostSuperbubblesAll.layout_bubblechains_all`` -- the scheme of po_layout_bubblechains_all run
synchronously, ring election included, through ``layout.bubble_chains(..., cyclic=True)`` -- and the ring-aware restatement
of the reference's walk against every application of tests/golden/bubblechain_all_cases.npz (tests/golden/
make_bubblechains_all_golden.py: both held equal there, and held against the reference's own build_bubblechains and
identify_contigs, executed), and what the contract promises on rings."""
import numpy as np
import pytest

import bubblechain_all_utils as ba
import bubblechain_utils as bu
import components_utils as cu
import contig_utils as ct
import cyclic_utils as cy
from phasm_amd import _lib, cyclic, layout
from test_contigs_oracle import CASES as CONTIG_CASES, stage_inputs as contig_stage_inputs

GOLDEN = ba.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids, min_nodes) for name, order, edges, n_ids, min_nodes in ba.direct_inputs()}
_CONTIG = {c["name"]: c for c in CONTIG_CASES}


def node_length(n):
    """The length of node n of a direct case: what tests/test_gpu_components.py segments() gives its segment."""
    return 1000 + (n >> 1) % 97


def stage_inputs(case):
    """{stage: (edges [n, 4], node order, n_ids, {node: length})} of a golden case: a direct case's own (weight 100), or the
    graphs of the text case at (b) and (c) as tests/test_contigs_oracle.py rebuilds them."""
    name = case["name"]
    if case.get("direct"):
        order, edges, _, _ = DIRECT[name[len("direct_"):]]
        e4 = np.asarray([(u, v, 100, 17) for u, v in edges], dtype=np.int64).reshape(-1, 4)
        return {"a": (e4, [int(n) for n in order], case["results"][0]["n_ids"], {int(n): node_length(int(n)) for n in order})}
    return contig_stage_inputs(_CONTIG[name])


def check_input(edges, order, lengths, rec):
    e = cu.uv_of(edges)
    by = np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, np.int64)
    assert cu.digest(order, e[by], np.asarray(edges, np.int64).reshape(-1, 4)[by, 2], [lengths[n] for n in order]) == rec["in_sha256"], \
        "the input differs from the generator's"


def exclude_of(res, order):
    """X of po_layout_contigs_all: the nodes that carry a chain."""
    return sorted(int(n) for n, c in zip(order, np.asarray(res["node_chain"]).tolist()) if c != ba.NONE)


def contig_check(res, crec, edges):
    """A ``contig_utils``-shaped result against a contig record of this golden (its digest starts at fewer edges)."""
    if "sha256" in crec and crec["n_edges"] <= ct.DIGEST_ABOVE:
        assert {k: int(res["stats"][k]) for k in ct.STAT_KEYS} == {k: crec[k] for k in ct.STAT_KEYS}
        assert cu.digest(*ct._canonical(res, edges)) == crec["sha256"]
    else:
        ct.check_against_record(res, crec, edges)


def host_result(edges, order, min_nodes):
    host = cyclic.HostSuperbubblesAll(edges, order)
    chains = layout.bubble_chains(host, None, min_nodes, cyclic=True)
    assert chains.node_order.tolist() == [int(x) for x in order] and chains.table.dtype == _lib.BUBBLECHAIN_DTYPE
    return ba.as_result(chains.stats, (chains.node_chain, chains.node_bubble, chains.edge_chain, chains.table)), chains


def test_one_parametrised_case_per_golden_case_and_the_situations():
    text = [c["name"] for c in cy.load_golden()["cases"] if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    assert len(text) == 111 and len(cy.direct_inputs()) == 109 and len(DIRECT) > 109
    t = GOLDEN["totals"]
    for k in ("ring_and_path_in_one_graph", "ring_with_nested_bubble", "ring_dropped_by_min_nodes", "power_of_two_ring",
              "ring_whose_leader_is_not_rank_0", "reference_one_bubble_short", "singleton_part_compared"):
        assert t[k] > 0, k
    assert t["with_a_ring_chain"] >= 20 and t["applications"] == 2 * len(text) + len(DIRECT)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_definition_and_host_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["b", "c"])
    for r in case["results"]:
        edges, order, n_ids, lengths = stages[r["stage"]]
        check_input(edges, order, lengths, r)
        assert r["n_ids"] == n_ids
        given = cu.uv_of(edges)[np.random.default_rng(len(edges)).permutation(len(edges))]     # (the edge order is no input of the contract)
        sync, chains = host_result(given.tolist(), order, r["min_nodes"])
        ba.check_against_record(sync, r, given)
        assert {k: int(sync["stats"][k]) for k in ba.SCHEME_KEYS} == {k: r[k] for k in ba.SCHEME_KEYS}
        plain = ba.definition(given, order, r["min_nodes"])
        ba.check_against_record(plain, r, given)
        st = sync["stats"]
        rank = {int(n): i for i, n in enumerate(order)}
        heads = [rank[s] for s in sync["c_first"].tolist()]
        assert heads == sorted(heads)                                          # numbered by the rank of their heads
        assert st["n_ring_rounds"] == (ba.ring_rounds(st["n_top"]) if st["n_top"] and st["n_cyclic_bubbles"] else 0)
        assert st["n_ring_chains"] <= st["n_chains"] + st["n_short"] and 2 * st["n_ring_chains"] <= st["n_ring_bubbles"] <= st["n_top"]
        rings = [j for j in range(len(heads)) if ba.is_ring(sync, j)]
        assert len(rings) <= st["n_ring_chains"] and (st["n_cyclic_bubbles"] > 0 or not rings)
        for j in range(len(heads)):
            walk = chains.bubbles_of(j)                                        # layout.BubbleChains on the same arrays
            assert len(walk) == sync["c_bubbles"][j] and walk[0][0] == sync["c_first"][j] and walk[-1][1] == sync["c_last"][j]
            assert len({s for s, _ in walk}) == len(walk)                      # a ring is walked once round
            assert [int(sync["node_bubble"][rank[s]]) for s, _ in walk] == list(range(len(walk)))
            if j in rings:                                                     # the head: the lowest-ranked entrance of the ring
                assert rank[walk[0][0]] == min(rank[s] for s, _ in walk)
        # the contigs outside these chains: the restatement of po_layout_contigs with X = the nodes of the chains
        X = exclude_of(sync, order)
        for crec in r["contigs"]:
            contig_check(ct.scheme(edges, order, lengths, X, crec["min_contig_len"]), crec, edges)


def test_what_the_contract_promises_on_rings():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    for k in (2, 3, 4, 5, 8, 15, 16, 17):
        for name, nodes in (("rc_ring_of_%d_%s" % (k, "diamonds" if k == 2 else "bubbles_scrambled"), 3 * k), ("rc_plain_ring_of_%d_descending" % k, k)):
            if name not in by:
                assert k == 2
                continue
            r = by[name]
            assert (r["n_chains"], r["n_ring_chains"], r["n_ring_bubbles"], r["n_chain_nodes"]) == (1, 1, k, nodes), name
            assert r["a_c_first"] == r["a_c_last"] and r["a_c_bubbles"] == [k] and r["n_ring_rounds"] == bu.log2_ceil(k) + 1
            assert set(r["a_node_chain"]) == {0} and sorted(set(r["a_node_bubble"])) == list(range(k))
    r = by["rc_ring_of_2_diamonds"]
    assert (r["n_nodes"], r["a_c_first"], r["a_c_last"], r["a_c_bubbles"], r["a_c_nodes"], r["a_c_edges"]) == (6, [0], [0], [2], [6], [8])
    assert r["a_node_bubble"] == [0, 0, 0, 1, 1, 1] and r["ref_short_rings"] == 1      # the reference: 4 of the 6 nodes
    r = by["rc_ring_lowest_rank_is_an_interior_node"]
    assert r["n_ring_chains"] == 1 and r["a_c_first"] == [0] and r["a_node_bubble"][0] != 0      # rank 0 is no entrance
    r = by["rc_ring_beside_a_path_chain"]
    assert (r["n_chains"], r["n_ring_chains"]) == (2, 1) and r["a_c_first"] == [100, 0] and r["a_c_last"] == [112, 0]
    r = by["rc_ring_with_a_nested_bubble"]
    assert r["n_ring_chains"] == 1 and r["n_bubbles"] == r["n_top"] + 1 and r["n_chain_nodes"] == r["n_nodes"] == 8
    r = by["rc_ring_dropped_by_min_nodes"]
    assert (r["n_chains"], r["n_short"], r["n_ring_chains"], r["n_ring_bubbles"]) == (1, 1, 1, 2) and r["a_c_first"] != r["a_c_last"]
    r = by["rc_ring_kept_path_chain_dropped"]
    assert (r["n_chains"], r["n_short"], r["n_ring_chains"]) == (1, 1, 1) and r["a_c_first"] == r["a_c_last"] == [0]
    r = by["rc_two_rings_joined_by_a_bridge"]
    assert r["n_ring_chains"] == 0 and r["n_cyclic_bubbles"] > 0 and r["n_ring_rounds"] > 0     # the election ran and found paths only
    for n in (257, 1025):                                                     # every edge of a plain ring is a trivial bubble
        r = by["ring_%d_ascending" % n]
        assert (r["n_ring_chains"], r["n_ring_bubbles"], r["max_chain_bubbles"], r["n_chain_nodes"]) == (1, n, n, n)
    assert by["cy_ring_of_3_diamonds"]["ref_short_rings"] == 1                 # the reference: 7 of the 9 nodes
    assert by["cy_strong_union_2000"]["n_ring_chains"] > 1000                  # most of the random strong components are rings


def test_without_a_cyclic_bubble_the_arrays_are_those_of_the_acyclic_call():
    import superbubble_utils as su
    seen = 0
    for c in CASES:
        for r in c["results"]:
            if r["n_cyclic_bubbles"] or r["n_nodes"] > 300 or "sha256" in r:
                continue
            edges, order, _, _ = stage_inputs(c)[r["stage"]]
            old = bu.scheme(edges, order, r["min_nodes"], su.scheme(edges, order))
            ba.check_against_record(old, r, edges, bu.STAT_KEYS)
            seen += 1
    assert seen >= 100


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    for f in (ba.definition, ba.scheme):
        with pytest.raises(ValueError):
            f(np.asarray([(0, 2), (2, 4)]), [0, 2])
    with pytest.raises(ValueError):
        cyclic.HostSuperbubblesAll([(0, 2)], [0, 2]).layout_bubblechains_all(None, 0)
