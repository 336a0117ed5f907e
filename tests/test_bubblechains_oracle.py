"""tests/bubblechain_utils.py -- the reference's sequential walk restated and the device's scheme run synchronously -- against
every application of tests/golden/bubblechain_cases.npz (tests/golden/make_bubblechains_golden.py: the reference's
build_bubblechains, unmodified, per qualifying weakly connected component of the reference's graphs at two stages and of the
direct cases), and ``layout.BubbleChains`` on outputs shaped as the device returns them."""
import numpy as np
import pytest

import bubblechain_utils as bu
import components_utils as cu
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_partition_oracle import CASES as PARTITION_CASES, stage_inputs as partition_stage_inputs

GOLDEN = bu.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids, min_nodes) for name, order, edges, n_ids, min_nodes in bu.direct_inputs()}
_PARTITION = {c["name"]: c for c in PARTITION_CASES}


def stage_inputs(case):
    """{stage: (edges [n, >=2], node order, n_ids)} of a golden case: a direct case's own, or the graphs of the text case at
    (b) and (c) as tests/test_partition_oracle.py rebuilds them."""
    name = case["name"]
    if case.get("direct"):
        order, edges, _, _ = DIRECT[name[len("direct_"):]]
        return {"a": (np.asarray(edges, dtype=np.int64).reshape(-1, 2), list(order), case["results"][0]["n_ids"])}
    return partition_stage_inputs(_PARTITION[name])


def check_input(edges, order, rec):
    e = cu.uv_of(edges)
    assert cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))]) == rec["in_sha256"], "the input differs from the generator's"


def as_device(res, order, sb):
    """The restatement's arrays in the dataclass the device route fills."""
    none = lambda a: np.where(np.asarray(a) < 0, _lib.NO_NODE, np.asarray(a)).astype(np.uint32)   # noqa: E731
    table = np.zeros(len(res["c_first"]), dtype=_lib.BUBBLECHAIN_DTYPE)
    for k, name in (("c_first", "first_entrance"), ("c_last", "last_exit"), ("c_bubbles", "n_bubbles"), ("c_nodes", "n_nodes"),
                    ("c_edges", "n_edges")):
        table[name] = res[k]
    return layout.BubbleChains(np.asarray(order, dtype=np.uint32), none(res["node_chain"]), none(res["node_bubble"]),
                               none(res["edge_chain"]), table, none(sb["node_exit"]), {})


def check_reference(res, edges, order, rec):
    """A ``definition``-shaped result against the (node set, edge count) of every chain the reference yielded on the
    components it was run on."""
    weak = cu.weak_components(edges, order)
    comp_of = dict(zip([int(x) for x in order], weak["node_component"].tolist()))
    on = set(rec["ref_components"])
    mine = sorted((sorted(bu.nodes_of(res, order, j)), k) for j, (first, k) in enumerate(zip(res["c_first"].tolist(), res["c_edges"].tolist()))
                  if comp_of[first] in on)
    if "ref_sha256" in rec:
        assert cu.digest([k for _, k in mine], [len(x) for x, _ in mine], [n for x, _ in mine for n in x]) == rec["ref_sha256"]
        return
    assert [k for _, k in mine] == list(rec["ref_chain_edges"])                      # networkx.number_of_edges(bubblechain)
    assert [len(x) for x, _ in mine] == list(rec["ref_chain_sizes"])                 # networkx.number_of_nodes(bubblechain)
    assert [n for x, _ in mine for n in x] == list(rec["ref_chain_nodes"])


def test_one_parametrised_case_per_golden_case_and_the_floors():
    text = [c["name"] for c in PARTITION_CASES if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    assert list(DIRECT)[:len(su.direct_inputs())] == [n for n, _, _, _ in su.direct_inputs()]    # the reused inputs, unchanged
    t = GOLDEN["totals"]
    assert t["applications"] == sum(len(c["results"]) for c in CASES) >= 301
    assert t["compared_with_the_reference"] >= 100 and t["with_a_chain_in_a_qualifying_component"] >= 50, t
    assert t["with_a_chain_of_at_least_2_bubbles"] >= 40 and t["longest_chain"] >= 1024, t
    assert all(t[k] > 0 for k in t if k != "digest_records"), t
    assert t["max_nest_rounds"] > 8 and t["max_chain_rounds"] > 8                                # both loops cross a batch


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_definition_and_device_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["b", "c"])
    for r in case["results"]:
        edges, order, n_ids = stages[r["stage"]]
        check_input(edges, order, r)
        assert r["n_ids"] == n_ids
        min_nodes = r["min_nodes"]
        assert min_nodes == (DIRECT[case["name"][len("direct_"):]][3] if case.get("direct") else 1)
        sb = su.scheme(edges, order)
        sync, plain = bu.scheme(edges, order, min_nodes, sb), bu.definition(edges, order, min_nodes, sb)
        rank = {int(n): i for i, n in enumerate(order)}
        for res in (sync, plain):
            bu.check_against_record(res, r, edges)
            check_reference(res, edges, order, r)
            first = [rank[s] for s in res["c_first"].tolist()]
            assert first == sorted(first)                                            # numbered by the rank of their heads
            assert all(n >= min_nodes for n in res["c_nodes"].tolist())
        st = sync["stats"]
        assert {k: st[k] for k in bu.SCHEME_KEYS} == {k: r[k] for k in bu.SCHEME_KEYS}
        nest_bound, chain_bound = bu.round_bounds(st)
        assert st["n_nest_rounds"] <= nest_bound and st["n_chain_rounds"] <= chain_bound
        assert st["n_chains"] + st["n_short"] <= st["n_top"] <= st["n_bubbles"]
        # layout.BubbleChains on the same arrays
        dev = as_device(sync, order, sb)
        assert len(dev) == st["n_chains"]
        uv = cu.uv_of(edges)
        for j in range(min(len(dev), 50)):
            nodes = dev.nodes_of(j).tolist()
            assert nodes == bu.nodes_of(sync, order, j) and len(nodes) == sync["c_nodes"][j]
            assert [rank[x] for x in nodes] == sorted(rank[x] for x in nodes)        # node order
            idx = dev.edges_of(j)
            assert idx.tolist() == sorted(idx.tolist()) and len(idx) == sync["c_edges"][j]     # edge order
            inside = set(nodes)
            assert idx.tolist() == [e for e, (u, v) in enumerate(uv.tolist()) if u in inside and v in inside]   # networkx.subgraph
            pairs = dev.bubbles_of(j)
            assert pairs == bu.bubbles_of(sync, order, sb, j) and len(pairs) == sync["c_bubbles"][j]
            assert pairs[0][0] == sync["c_first"][j] and pairs[-1][1] == sync["c_last"][j]
            assert all(a[1] == b[0] for a, b in zip(pairs, pairs[1:]))                # linked
            top = set(zip(sb["b_entrance"][sb["b_nested"] == 0].tolist(), sb["b_exit"][sb["b_nested"] == 0].tolist()))
            assert set(pairs) <= top
            for k, (s, t) in enumerate(pairs):                                       # the positions the contract names
                assert sync["node_bubble"][rank[s]] == k and sync["node_bubble"][rank[t]] == (k if k + 1 == len(pairs) else k + 1)


def test_the_shapes_the_direct_cases_are_about():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    count = lambda name: (by[name]["n_chains"], by[name]["n_short"], by[name]["n_top"])   # noqa: E731
    table = lambda name: list(zip(by[name]["a_c_first"], by[name]["a_c_last"], by[name]["a_c_bubbles"], by[name]["a_c_nodes"],   # noqa: E731
                                  by[name]["a_c_edges"]))
    assert count("bc_two_chains_heads_descending") == (2, 0, 4)
    assert table("bc_two_chains_heads_descending") == [(20, 24, 2, 3, 2), (0, 4, 2, 3, 2)]     # the head of rank 0 first, whatever its id
    assert table("bc_head_with_and_without_in_edges") == [(0, 4, 2, 3, 2), (10, 14, 2, 3, 2)]
    assert count("sb_two_diamonds_sharing_a_node") == (1, 0, 2) and table("sb_two_diamonds_sharing_a_node") == [(0, 12, 2, 7, 8)]
    assert by["sb_two_diamonds_sharing_a_node"]["a_node_bubble"] == [0, 0, 0, 1, 1, 1, 1]       # the shared node enters the second
    assert table("bc_diamond_edge_diamond_fork") == [(0, 14, 3, 8, 9)]                         # 3 bubbles, 8 nodes, 9 edges
    assert sorted(by["bc_diamond_edge_diamond_fork"]["a_node_chain"]) == [bu.NONE] * 2 + [0] * 8
    r = by["bc_nesting_depth_3_inside_a_chain_member"]
    assert (r["n_bubbles"], r["n_top"], r["n_chains"], r["max_chain_bubbles"]) == (8, 3, 1, 3)  # inner bubbles make no chain
    assert table("bc_nesting_depth_3_inside_a_chain_member") == [(40, 46, 3, 17, 20)] and r["n_nest_rounds"] == 3   # 4 + 12 + 1 nodes, 4 + 15 + 1 edges
    r = by["bc_nesting_depth_300"]
    assert (r["n_bubbles"], r["n_top"], r["n_chains"]) == (300, 1, 1) and table("bc_nesting_depth_300") == [(0, 2, 1, 600, 898)]
    assert r["n_nest_rounds"] == 10 > 8                                                        # crosses a batch
    for n, doublings in ((257, 8), (1025, 10)):
        for tag in ("ascending", "descending", "scrambled"):
            name = ("bc_path_%d_%s" if n == 257 else "sb_path_%d_%s") % (n, tag)
            assert count(name) == (1, 0, n - 1) and table(name) == [(0, 2 * (n - 1), n - 1, n, n - 1)]
            assert by[name]["n_chain_rounds"] == doublings + 1 and by[name]["max_chain_bubbles"] == n - 1
            ids = DIRECT[name][0]
            assert [by[name]["a_node_bubble"][ids.index(2 * i)] for i in (0, 1, n - 2, n - 1)] == [0, 1, n - 2, n - 2]
    assert table("bc_self_loop_on_a_middle_node_of_a_path") == [(0, 6, 3, 4, 3), (10, 16, 3, 4, 3)]   # splits the chain in two
    assert by["bc_self_loop_on_a_middle_node_of_a_path"]["a_node_chain"] == [0, 0, 0, 0, bu.NONE, 1, 1, 1, 1]
    assert table("sb_nested_with_the_outer_one_discarded") == [(4, 10, 1, 4, 4), (16, 14, 1, 2, 1)]
    assert table("sb_fan_out_and_in_257") == [(0, 2, 1, 259, 514)]
    r = by["sb_disjoint_edges_2050"]
    assert count("sb_disjoint_edges_2050") == (2050, 0, 2050) and (r["n_chain_nodes"], r["n_chain_edges"]) == (4100, 2050)
    assert count("bc_min_nodes_3_on_disjoint_edges_plus_a_diamond") == (1, 5, 6)
    assert table("bc_min_nodes_3_on_disjoint_edges_plus_a_diamond") == [(100, 106, 1, 4, 4)]
    assert by["bc_min_nodes_3_on_disjoint_edges_plus_a_diamond"]["a_node_chain"] == [bu.NONE] * 10 + [0] * 4
    assert count("bc_min_nodes_above_every_chain") == (0, 6, 6) and by["bc_min_nodes_above_every_chain"]["n_chain_nodes"] == 0
    r = by["bc_min_nodes_above_every_chain_of_a_long_path"]
    assert count("bc_min_nodes_above_every_chain_of_a_long_path") == (0, 1, 39) and r["max_chain_bubbles"] == 39
    assert table("three_cycle_with_tails") == [] and by["three_cycle_with_tails"]["n_top"] == 0
    assert count("empty") == (0, 0, 0) and by["empty"]["n_nodes"] == 0


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    for f in (bu.definition, bu.scheme):
        with pytest.raises(ValueError):
            f([(0, 2), (2, 4)], [0, 2])
