"""The contract of po_phase_paths without a GPU: tests/paths_utils.py ``definition`` (plain Python), ``scheme`` (the device's
scheme in numpy) and ``phasm_amd.phasing.HostPaths`` against tests/golden/paths_cases.npz, which make_paths_golden.py held to the
reference's find_superbubbles and superbubble_nodes, to networkx.all_simple_paths and to predecessors_iter; every bubble of
every walk of walk_cases.npz -- what the reference's phase() computed on its own graph -- for paths, interior_nodes, preds and the
visiting order."""
import numpy as np
import pytest

import paths_utils as pp
import walk_utils as wu
from phasm_amd import _lib, phasing

CASES = pp.load_golden()["cases"]
WALKS = [c for c in CASES if "walk" in c]
BY_NAME = {c["name"]: c for c in CASES}


def test_the_golden_holds_the_cases_the_contract_is_about():
    names = set(BY_NAME)
    assert len(WALKS) == len(wu.load_golden()["walks"]) == 11
    for wanted in ("direct_nested_in_nested", "direct_exit_in_degree_1", "direct_exit_in_degree_2", "direct_exit_in_degree_65",
                   "direct_permuted_0", "direct_permuted_1", "direct_permuted_2", "direct_direct_edge_first", "direct_direct_edge_middle",
                   "direct_direct_edge_last", "direct_bare_in_the_middle", "direct_two_chains", "direct_exactly_max_paths",
                   "direct_max_paths_plus_one", "direct_saturated_64", "direct_unlisted_62", "direct_one_bubble_129_paths"):
        assert wanted in names, wanted
    flags = lambda name: BY_NAME[name]["result"]["b_flags"]   # noqa: E731
    paths = lambda name: [int(x) for x in BY_NAME[name]["result"]["b_paths"]]   # noqa: E731
    assert paths("direct_saturated_64") == [pp.MANY] and flags("direct_saturated_64") == [pp.UNLISTED | pp.SATURATED]
    assert paths("direct_unlisted_62") == [2**62 + 1] and flags("direct_unlisted_62") == [pp.UNLISTED]
    assert paths("direct_exactly_max_paths") == [9] and flags("direct_exactly_max_paths") == [0]
    assert paths("direct_max_paths_plus_one") == [9] and flags("direct_max_paths_plus_one") == [pp.UNLISTED]
    assert paths("direct_one_bubble_129_paths") == [129] and flags("direct_one_bubble_129_paths") == [0]
    # interior and predecessors stay exact where nothing is listed
    sat = BY_NAME["direct_saturated_64"]["result"]
    assert sat["b_inside"] == [64 * 3 + 2] == [len(sat["inside_nodes"])] and len(sat["pred_node"]) == 2 and sat["path_nodes"] == []
    # the three permutations list the same set of paths in three different orders
    lists = []
    for k in range(3):
        r = pp.result_of_record(BY_NAME["direct_permuted_%d" % k]["result"])
        off = r["path_off"]
        lists.append([tuple(r["path_nodes"][off[p]:off[p + 1]].tolist()) for p in range(int(r["bubble_path_off"][1]))])
    assert len({tuple(x) for x in lists}) == 3 and len({frozenset(x) for x in lists}) == 1
    # a bare bubble with bubbles behind it; two chains
    bare = BY_NAME["direct_bare_in_the_middle"]["result"]
    assert bare["b_flags"] == [0, 0, pp.BARE, 0, 0] and bare["b_chain"] == [0] * 5 and bare["b_position"] == list(range(5))
    assert sorted(set(BY_NAME["direct_two_chains"]["result"]["b_chain"])) == [0, 1]
    # the direct edge s -> t is path 0, 1 and 2
    for k, where in enumerate(("first", "middle", "last")):
        r = BY_NAME["direct_direct_edge_" + where]["result"]
        assert [r["path_off"][p + 1] - r["path_off"][p] for p in range(3)].index(2) == k


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_definition_scheme_and_host_paths_equal_the_golden(case):
    order, edges, max_paths = pp.case_inputs(case)
    want = pp.result_of_record(case["result"])
    d = pp.definition(edges, order, max_paths)
    pp.same(d, want)
    s = pp.scheme(edges, order, max_paths)
    pp.same(s, want)
    assert s["stats"]["n_count_rounds"] == want["stats"]["n_count_rounds"] <= max(want["b_inside"].tolist() + [-2]) + 2
    assert want["stats"]["n_stray_edges"] == 0
    host = phasing.HostPaths(edges, order)
    bp = host.phase_paths(None, max_paths)
    pp.same(pp.result_of(bp, host.paths_stats()), want)
    assert bp.bubbles.dtype == _lib.BUBBLE_PATHS_DTYPE and bp.path_nodes.dtype == np.uint32 and bp.path_off.dtype == np.uint64
    # the invariants of the table
    for b in range(len(bp)):
        row = bp.bubbles[b]
        flags = int(row["flags"])
        assert bool(flags & pp.BARE) == (row["n_inside"] == 0) == bp.is_bare(b)
        assert bool(flags & pp.UNLISTED) == (int(row["n_paths"]) > max_paths or bool(flags & pp.SATURATED))
        assert bool(flags & pp.SATURATED) == (int(row["n_paths"]) == pp.MANY)
        assert len(bp.interior_of(b)) == row["n_inside"]
        if flags & pp.UNLISTED:
            assert row["n_path_nodes"] == 0 and bp.bubble_path_off[b] == bp.bubble_path_off[b + 1]
            with pytest.raises(ValueError):
                bp.paths_of(b)
        else:
            paths = bp.paths_of(b)
            assert len(paths) == row["n_paths"] == len(set(paths)) and sum(map(len, paths)) == row["n_path_nodes"]
            assert all(p[0] == row["entrance"] and p[-1] == row["exit"] and set(p[1:-1]) <= set(bp.interior_of(b)) for p in paths)
        assert all(p in bp.interior_of(b) or p == row["entrance"] for p, _ in bp.preds_of(b))


@pytest.mark.parametrize("case", WALKS, ids=[c["name"] for c in WALKS])
def test_every_bubble_of_a_walk_as_phase_computed_it(case):
    walk = wu.load_golden()["walks"][case["walk"]]
    order, edges, max_paths = pp.case_inputs(case)
    assert edges == [list(e) for e in wu.edges_of(walk)] and order == pp.first_seen(edges)
    for src in (phasing.HostPaths(edges, order),):
        bp = phasing.bubble_paths(src, None, max_paths)
        visited = bp.chain_bubbles(0)
        assert set(bp.bubbles["chain"].tolist()) == {0}
        assert [int(bp.bubbles["entrance"][b]) for b in visited] == [x["entrance"] for x in walk["bubbles"]]     # the visiting order
        for b, want in zip(visited, walk["bubbles"]):
            assert int(bp.bubbles["exit"][b]) == want["exit"]
            assert [list(p) for p in bp.paths_of(b)] == want["paths"]
            assert bp.interior_of(b) == sorted(want["interior_nodes"], key=order.index)
            assert [list(p) for p in bp.preds_of(b)] == want["preds"]
            large = len(want["paths"]) > walk["params"]["max_bubble_size"]
            assert bp.is_large(b, walk["params"]["max_bubble_size"]) == large
    # counts only: the decision needs no listing
    counted = phasing.HostPaths(edges, order).phase_paths(None, 0)
    assert counted.bubbles["n_paths"].tolist() == bp.bubbles["n_paths"].tolist() and len(counted.path_nodes) == 0


def test_chain_bubbles_stop_at_the_first_bare_bubble():
    order, edges, max_paths = pp.case_inputs(BY_NAME["direct_bare_in_the_middle"])
    bp = phasing.HostPaths(edges, order).phase_paths(None, max_paths)
    assert bp.chain_bubbles(0) == [0, 1] and bp.chain_bubbles(1) == []
    order, edges, max_paths = pp.case_inputs(BY_NAME["direct_two_chains"])
    bp = phasing.HostPaths(edges, order).phase_paths(None, max_paths)
    assert bp.chain_bubbles(0) == [0, 1] and bp.chain_bubbles(1) == [5, 6, 7]


def test_capacity_is_decided_from_the_counts():
    order, edges, _ = pp.case_inputs(BY_NAME["direct_unlisted_62"])
    with pytest.raises(pp.Capacity):
        pp.definition(edges, order, 2**62 + 1)
    with pytest.raises(pp.Capacity):
        pp.scheme(edges, order, 2**62 + 1)
    with pytest.raises(OverflowError, match="paths to list"):
        phasing.HostPaths(edges, order).phase_paths(None, 2**62 + 1)
    with pytest.raises(ValueError):
        phasing.HostPaths([(0, 5, 1)], [0, 1])
    assert phasing.paths_text(pp.MANY) == ">=2^64-1" and phasing.paths_text(9) == "9"


def test_union_expectation_equals_the_scheme_where_that_is_cheap():
    """The broadcast that the scale test trusts, held to ``scheme`` itself on three copies, both layouts."""
    cases = [BY_NAME[n] for n in pp.UNION_NAMES]
    for layout in ("copy_major", "interleaved"):
        order, edges, want = pp.union_of(cases, 3, layout)
        got = pp.scheme(edges.tolist(), order.tolist(), 200)
        for k in pp.ARRAY_KEYS:
            assert np.array_equal(got[k], want[k]), (layout, k)
