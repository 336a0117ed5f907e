"""tests/superbubble_utils.py -- the definition of a superbubble by brute force and the device's scheme run synchronously --
against every application of tests/golden/superbubble_cases.npz (tests/golden/make_superbubbles_golden.py: the reference's
partition_graph, SuperBubbleFinderDAG and superbubble_nodes, unmodified, per weakly connected component of the reference's
graphs at two stages and of the direct cases), and ``layout.Superbubbles`` on outputs shaped as the device returns them."""
import numpy as np
import pytest

import components_utils as cu
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_partition_oracle import CASES as PARTITION_CASES, stage_inputs as partition_stage_inputs

GOLDEN = su.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids) for name, order, edges, n_ids in su.direct_inputs()}
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


def as_device(res, order):
    """The restatement's arrays in the dataclass the device route fills."""
    none = lambda a: np.where(np.asarray(a) < 0, _lib.NO_NODE, np.asarray(a)).astype(np.uint32)   # noqa: E731
    table = np.zeros(len(res["b_entrance"]), dtype=_lib.SUPERBUBBLE_DTYPE)
    for k, name in (("b_entrance", "entrance"), ("b_exit", "exit"), ("b_inside", "n_inside"), ("b_nested", "nested")):
        table[name] = res[k]
    return layout.Superbubbles(np.asarray(order, dtype=np.uint32), none(res["node_exit"]), none(res["node_inside"]),
                               res["node_flags"].astype(np.uint8), table, {})


def check_reference(res, sets, edges, order, rec):
    """A ``definition``-shaped result and the node set of every bubble (table order) against what the reference reported on
    the components it was run on."""
    weak = cu.weak_components(edges, order)
    comp_of = dict(zip([int(x) for x in order], weak["node_component"].tolist()))
    on = set(rec["ref_components"])
    mine = sorted((s, t, nested, nodes) for s, t, nested, nodes in zip(res["b_entrance"].tolist(), res["b_exit"].tolist(),
                                                                      res["b_nested"].tolist(), sets) if comp_of[s] in on)
    pairs, top = [(s, t) for s, t, _, _ in mine], [(s, t) for s, t, nested, _ in mine if not nested]
    if "ref_sha256" in rec:
        assert cu.digest(pairs, top, [len(x[3]) for x in mine], [n for x in mine for n in x[3]]) == rec["ref_sha256"]
        return
    flat = lambda ps: [x for p in ps for x in p]   # noqa: E731
    assert flat(pairs) == list(rec["ref_pairs"])                      # SuperBubbleFinderDAG(partition, True)
    assert flat(top) == list(rec["ref_top"])                          # SuperBubbleFinderDAG(partition, False)
    assert [len(x[3]) for x in mine] == list(rec["ref_set_sizes"])    # superbubble_nodes(component, s, t)
    assert [n for x in mine for n in x[3]] == list(rec["ref_set_nodes"])


def test_one_parametrised_case_per_golden_case():
    text = [c["name"] for c in PARTITION_CASES if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    t = GOLDEN["totals"]
    assert t["compared_with_the_reference"] >= 100 and t["compared_and_with_a_bubble"] >= 40, t
    free = ("digest_records", "direct_cases_where_the_finder_depends_on_the_order")
    assert all(t[k] > 0 for k in t if k not in free), t
    assert t["max_levels"] >= 1025


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_definition_and_device_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["b", "c"])
    for r in case["results"]:
        edges, order, n_ids = stages[r["stage"]]
        check_input(edges, order, r)
        assert r["n_ids"] == n_ids
        sync = su.scheme(edges, order)
        results = [sync] + ([su.definition(edges, order)] if len(order) <= su.BRUTE_FORCE_UP_TO else [])
        for res in results:
            su.check_against_record(res, r)
            check_reference(res, su.node_sets(res, order), edges, order, r)
            rank = {int(n): i for i, n in enumerate(order)}
            first = [rank[s] for s in res["b_entrance"].tolist()]
            assert first == sorted(first)                                            # the table's order: the entrances' ranks
            assert len(set(res["b_exit"].tolist())) == len(first)                    # a node exits at most one bubble
        st = sync["stats"]
        assert {k: st[k] for k in su.SCHEME_KEYS} == {k: r[k] for k in su.SCHEME_KEYS}
        n_real = st["n_p_nodes"]
        assert st["n_levels_forward"] <= n_real and st["n_level_rounds"] <= 2 * (n_real + 2) and st["n_discard_rounds"] <= n_real + 2
        # layout.Superbubbles on the same arrays: pairs() and nodes() are the reference's
        dev = as_device(sync, order)
        assert dev.pairs() == list(zip(sync["b_entrance"].tolist(), sync["b_exit"].tolist())) and len(dev) == st["n_bubbles"]
        assert dev.pairs(nested=False) == [p for p, nested in zip(dev.pairs(), sync["b_nested"].tolist()) if not nested]
        check_reference(sync, [sorted(dev.nodes(s).tolist()) for s, _ in dev.pairs()], edges, order, r)
        for (s, _), k in zip(dev.pairs()[:50], sync["b_inside"].tolist()):
            assert sorted(dev.nodes(s).tolist()) == sorted(su.nodes_of(sync, order, s)) and len(dev.nodes(s)) == k + 2


def test_the_shapes_the_direct_cases_are_about():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    count = lambda name: (by[name]["n_bubbles"], by[name]["n_nested"], by[name]["n_discarded"])   # noqa: E731
    assert count("empty") == (0, 0, 0) and by["empty"]["n_p_nodes"] == 0
    assert count("every_node_in_a_cycle") == (0, 0, 0) and by["every_node_in_a_cycle"]["n_p_nodes"] == 0   # the empty acyclic partition
    assert count("sb_single_edge") == (1, 0, 0) and count("sb_path_3") == (2, 0, 0)        # one trivial bubble per edge
    for n in (9, 17, 1025):
        for tag in ("ascending", "descending", "scrambled"):
            r = by["sb_path_%d_%s" % (n, tag)]
            assert count("sb_path_%d_%s" % (n, tag)) == (n - 1, 0, 0)
            assert r["n_levels_forward"] == r["n_levels_backward"] == n and r["n_level_rounds"] == 2 * n   # > 8, > 16 rounds, 1 025 levels
    assert count("sb_diamond") == (1, 0, 0) and by["sb_diamond"]["a_b_inside"] == [2]
    assert count("sb_diamond_with_a_chord") == (1, 0, 0) and by["sb_diamond_with_a_chord"]["n_levels_forward"] == 4
    r = by["sb_branches_1_2_5"]                                                            # the outer bubble and the chains' edges
    assert count("sb_branches_1_2_5") == (6, 5, 0) and max(r["a_b_inside"]) == 8
    assert count("sb_two_diamonds_sharing_a_node") == (2, 0, 0)
    assert sum(f & 3 == 3 for f in by["sb_two_diamonds_sharing_a_node"]["a_node_flags"]) == 1      # exit = entrance
    r = by["sb_nesting_depth_3"]
    inside = dict(zip(DIRECT["sb_nesting_depth_3"][0], r["a_node_inside"]))
    chain = [14]
    while inside[chain[-1]] != su.NONE:
        chain.append(inside[chain[-1]])
    assert chain == [14, 12, 8, 2] and count("sb_nesting_depth_3") == (8, 5, 0)           # three bubbles around node 14
    assert count("sb_self_loop_inside_nesting_depth_3") == (5, 0, 3) and by["sb_self_loop_inside_nesting_depth_3"]["n_discard_rounds"] == 3
    r = by["sb_nested_with_the_outer_one_discarded"]                                       # the inner one survives, not NESTED
    assert count("sb_nested_with_the_outer_one_discarded") == (2, 0, 1) and r["n_survivors_in_discarded"] == 1
    assert (4, 10) in list(zip(r["a_b_entrance"], r["a_b_exit"]))
    for name in ("sb_tip_inside", "sb_in_edge_from_outside", "sb_out_edge_into_a_cycle", "sb_in_edge_from_a_cycle"):
        assert count(name) == (0, 0, 0)
    assert count("sb_self_loop_on_the_entrance") == (1, 0, 2) and by["sb_self_loop_on_the_entrance"]["a_b_entrance"] == [6]
    assert count("sb_self_loop_on_the_exit") == (1, 0, 2) and by["sb_self_loop_on_the_exit"]["a_b_entrance"] == [10]
    assert count("sb_self_loop_on_the_interior") == (2, 0, 1) and by["sb_self_loop_on_the_interior"]["a_b_entrance"] == [10, 6]
    assert count("sb_lone_self_loop") == (0, 0, 0) and by["sb_lone_self_loop"]["n_self_loop_nodes"] == 1
    assert count("sb_self_loop_as_the_only_out_edge") == (1, 0, 0) and by["sb_self_loop_as_the_only_out_edge"]["a_b_entrance"] == [4]
    assert count("sb_fan_in_257") == (0, 0, 0) and count("sb_fan_out_257") == (0, 0, 0)
    assert count("sb_fan_out_and_in_257") == (1, 0, 0) and by["sb_fan_out_and_in_257"]["a_b_inside"] == [257]
    assert count("sb_disjoint_edges_2050") == (2050, 0, 0)
    assert sum(1 for n in by if n.startswith("sb_random_dag_200_")) == 10 and sum(1 for n in by if n.startswith("sb_random_digraph_200_")) == 5
    assert all(by[n]["n_bubbles"] > 0 for n in by if n.startswith("sb_random_"))


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    for f in (su.definition, su.scheme):
        with pytest.raises(ValueError):
            f([(0, 2), (2, 4)], [0, 2])
