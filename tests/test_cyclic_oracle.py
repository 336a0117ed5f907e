"""``phasm_amd.cyclic.HostSuperbubblesAll`` -- the scheme of po_layout_superbubbles_all run synchronously, through
``layout.superbubbles(..., cyclic=True)`` -- against every application of tests/golden/superbubble_all_cases.npz
(tests/make_cyclic_golden.py: the definition by brute force on the whole graph, the same per partition, and the scheme, held
equal on every application small enough), and the run counts the scheme promises on rings."""
import numpy as np
import pytest

import components_utils as cu
import cyclic_utils as cy
import partition_utils as pu
from phasm_amd import _lib, cyclic, layout
from test_partition_oracle import CASES as PARTITION_CASES, stage_inputs as partition_stage_inputs

GOLDEN = cy.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids) for name, order, edges, n_ids in cy.direct_inputs()}
_PARTITION = {c["name"]: c for c in PARTITION_CASES}


def stage_inputs(case):
    """{stage: (edges [n, >=2], node order, n_ids)} of a golden case: a direct case's own, or the graphs of the text case at
    (b) and (c) as tests/test_partition_oracle.py rebuilds them."""
    name = case["name"]
    if case.get("direct"):
        order, edges, _ = DIRECT[name[len("direct_"):]]
        return {"a": (np.asarray(edges, dtype=np.int64).reshape(-1, 2), list(order), case["results"][0]["n_ids"])}
    return partition_stage_inputs(_PARTITION[name])


def check_input(edges, order, rec):
    e = cu.uv_of(edges)
    assert cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))]) == rec["in_sha256"], "the input differs from the generator's"


def host_result(edges, order):
    host = cyclic.HostSuperbubblesAll(edges, order)
    sb = layout.superbubbles(host, None, cyclic=True)
    assert sb.node_order.tolist() == [int(x) for x in order] and sb.table.dtype == _lib.SUPERBUBBLE_DTYPE
    return cy.as_result(sb.stats, (sb.node_exit, sb.node_inside, sb.node_flags, sb.table)), sb, host


def test_one_parametrised_case_per_golden_case():
    text = [c["name"] for c in PARTITION_CASES if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    t = GOLDEN["totals"]
    for k in ("rootless_first_root_certified", "rootless_two_or_more_runs", "cycle_exhausted_without_a_certificate",
              "three_or_more_split_levels", "edge_filter_fired", "split_node_as_entrance", "split_node_as_exit",
              "node_inside_from_a_later_run", "brute_forced", "with_a_cyclic_bubble"):
        assert t[k] > 0, k
    assert t["brute_forced"] >= 300 and t["applications"] == 2 * len(text) + len(DIRECT)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_host_scheme_equals_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["b", "c"])
    for r in case["results"]:
        edges, order, n_ids = stages[r["stage"]]
        check_input(edges, order, r)
        assert r["n_ids"] == n_ids
        uv = cu.uv_of(edges).tolist()
        res, sb, host = host_result(cy.scrambled_edges(uv), order)           # (the edge order is no input of the contract)
        cy.check_against_record(res, r)
        rank = {int(n): i for i, n in enumerate(order)}
        first = [rank[s] for s in res["b_entrance"].tolist()]
        assert first == sorted(first)                                         # the table's order: the entrances' ranks
        assert len(set(res["b_exit"].tolist())) == len(first)                 # a node exits at most one bubble
        st = res["stats"]
        assert st["n_certified"] <= st["n_rootless"] and st["n_split_levels"] <= st["n_split"] <= st["n_nodes"]
        assert (st["n_root_runs"] >= 1) == (len(order) > 0) and (st["n_root_runs"] <= 1 or st["n_rootless"] > 0)
        assert st["n_bubbles"] - st["n_cyclic_bubbles"] == r["n_acyclic_bubbles"]
        assert [run[min(run)] for run in host.roots_of_runs if run] == list(r["roots_of_first_rootless"])
        # layout.Superbubbles on the same arrays: pairs() and nodes() read them as they read po_layout_superbubbles'
        assert sb.pairs() == list(zip(res["b_entrance"].tolist(), res["b_exit"].tolist())) and len(sb) == st["n_bubbles"]
        for (s, _), k in list(zip(sb.pairs(), res["b_inside"].tolist()))[:50]:
            assert len(sb.nodes(s)) == k + 2


def test_the_run_counts_on_rings():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    runs = lambda name: (by[name]["n_rootless"], by[name]["n_root_runs"], by[name]["n_certified"])   # noqa: E731
    # a ring rooted at an end node of a bubble: one run, certified
    for name in ("cy_three_ring", "cy_ring_with_a_diamond_lowest_is_the_entrance", "cy_ring_with_a_diamond_lowest_is_the_exit",
                 "cy_ring_with_a_diamond_lowest_is_the_outside", "cy_ring_of_3_diamonds", "cy_ring_of_16_diamonds", "ring_257_ascending",
                 "ring_257_scrambled", "ring_1025_ascending", "ring_1025_scrambled"):
        assert runs(name) == (1, 1, 1), name
        assert by[name]["n_split"] == 1 and by[name]["n_split_levels"] == 1
    # ... at the interior of a simple diamond: the bubble's exit is one step along the cycle, so two runs
    for name in ("cy_ring_with_a_diamond_lowest_is_the_interior", "cy_ring_of_3_diamonds_interior_lowest", "cy_ring_of_16_diamonds_interior_lowest"):
        assert runs(name) == (1, 2, 1), name
    for n in (257, 1025):                                                     # every edge of a ring is a trivial bubble
        for tag in ("ascending", "scrambled"):
            r = by["ring_%d_%s" % (n, tag)]
            assert (r["n_bubbles"], r["n_cyclic_bubbles"], r["n_nested"]) == (n, n, 0)
    assert (by["cy_two_cycle"]["n_bubbles"], by["cy_two_cycle"]["n_edge_filtered"]) == (0, 2)                # (0, 1) and (1, 0) both go
    assert by["every_node_in_a_cycle"]["n_bubbles"] == 3 and by["every_node_in_a_cycle"]["n_acyclic_bubbles"] == 0
    assert by["k8_both_directions"]["n_split_levels"] == 7 and by["k8_both_directions"]["n_bubbles"] == 0
    assert by["two_cycles_2050"]["n_rootless"] == 2050 and by["two_cycles_2050"]["n_split"] == 2050
    for low in range(7):                                                      # the 7-node case: (1, 3), whatever the lowest rank
        r = by["cy_seven_nodes_lowest_%d" % low]
        assert (r["a_b_entrance"], r["a_b_exit"]) == ([2], [6]) and r["n_root_runs"] >= 2
        assert r["roots_of_first_rootless"][0] == 0 and len(r["roots_of_first_rootless"]) == r["n_root_runs"]   # (ranks: the lowest first)
    r = by["cy_four_node_digraphs_4096"]
    assert r["n_nodes"] == 16384 and r["n_split"] > 4096 and r["n_rootless"] > 0 and "sha256" in r
    r = by["cy_strong_union_2000"]
    assert r["n_rootless"] == 2000 and r["n_cyclic_bubbles"] == r["n_bubbles"] > 0 and r["n_root_runs"] >= 3


def test_the_four_node_union_is_brute_forced_per_copy():
    """All 4 096 loop-free digraphs on 4 labelled nodes in one graph: the scheme on the union against the definition on every
    copy by itself."""
    order, edges = cy.four_node_union()
    res, _, _ = host_result(edges, order)
    got = dict(zip(res["b_entrance"].tolist(), res["b_exit"].tolist()))
    slots = [(a, b) for a in range(4) for b in range(4) if a != b]
    want = {}
    for k in range(4096):
        mine = [(a, b) for i, (a, b) in enumerate(slots) if k >> i & 1]
        for s, (t, _) in cy.brute_force(4, mine, range(4)).items():
            want[8 * k + 2 * s] = 8 * k + 2 * t
    assert got == want and len(want) == 1008


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    for f in (cy.definition_all, cy.by_partition, cy.scheme_all):
        with pytest.raises(ValueError):
            f([(0, 2), (2, 4)], [0, 2])
    assert pu.R_IN == 1   # (the flags the scheme's roots are named after)
