"""tests/contig_utils.py -- the reference's sequential queue walk restated and the device's scheme run synchronously -- against
every application of tests/golden/contig_cases.npz (tests/golden/make_contigs_golden.py: the reference's identify_contigs,
unmodified, on the reference's graphs at two stages with the nodes of the bubble chains excluded, for two minimum lengths, and
on the direct cases), and ``layout.Contigs`` on outputs shaped as the device returns them."""
import numpy as np
import pytest

import bubblechain_utils as bu
import components_utils as cu
import contig_utils as ct
import merge_utils as mu
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs, _MERGE
from test_merge_oracle import node_lengths

GOLDEN = ct.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: rest for name, *rest in ct.direct_inputs()}
_STAGES = {}
_COMPONENTS = {c["name"]: c for c in COMPONENT_CASES}


def stage_inputs(case):
    """{stage: (edges [n, 4], node order, n_ids, {node: length})} of a golden case: a direct case's own, or the graphs of the
    text case at (b) and (c) as tests/test_components_oracle.py rebuilds them, with the lengths of the reads and, for the
    merged nodes, the lengths the merge gives them."""
    name = case["name"]
    if name in _STAGES:
        return _STAGES[name]
    if case.get("direct"):
        order, edges, lengths, _, _ = DIRECT[name[len("direct_"):]]
        e4 = np.asarray([(u, v, w, 17) for u, v, w in edges], dtype=np.int64).reshape(-1, 4)
        out = {"a": (e4, list(order), case["results"][0]["n_ids"], dict(lengths))}
    else:
        stages = component_stage_inputs(_COMPONENTS[name])
        L = node_lengths(_MERGE[name])
        e_b, order_b, n_ids = stages["b"]
        merged = mu.merge_paths(e_b, order_b, L, n_ids)
        lengths = {n: int(x) for n, x in enumerate(L)}
        lengths.update({n_ids + k: int(x) for k, x in enumerate(merged["lengths"].tolist())})
        out = {k: (np.asarray(stages[k][0], dtype=np.int64).reshape(-1, 4), [int(n) for n in stages[k][1]], n_ids, lengths) for k in ("b", "c")}
    _STAGES[name] = out
    return out


def check_input(edges, order, lengths, exclude, rec):
    e = cu.uv_of(edges)
    by = np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, np.int64)
    assert cu.digest(order, e[by], np.asarray(edges, np.int64).reshape(-1, 4)[by, 2], [lengths[n] for n in order], sorted(exclude)) == \
        rec["in_sha256"], "the input differs from the generator's"


def exclude_of(case, rec):
    return DIRECT[case["name"][len("direct_"):]][3] if case.get("direct") else rec["exclude"]


def as_device(res, order, edges):
    """The restatement's arrays in the dataclass the device route fills."""
    none = lambda a: np.where(np.asarray(a) < 0, _lib.NO_NODE, np.asarray(a)).astype(np.uint32)   # noqa: E731
    table = np.zeros(len(res["c_first"]), dtype=_lib.CONTIG_DTYPE)
    for k, name in (("c_first", "first_node"), ("c_last", "last_node"), ("c_nodes", "n_nodes"), ("c_length", "length")):
        table[name] = res[k]
    table["first_edge"] = none(res["c_first_edge"])
    return layout.Contigs(np.asarray(order, dtype=np.uint32), none(res["edge_contig"]), none(res["edge_pos"]), table, {},
                          cu.uv_of(edges).astype(np.uint32).reshape(-1, 2))


def check_reference(res, edges, rec):
    """A ``definition``-shaped result against the paths the reference yielded, as sorted lists of node tuples."""
    mine = sorted(ct.paths_of(res, edges))
    assert len(set(mine)) == len(mine)                                               # no path twice
    flat = [n for p in mine for n in p]
    if "ref_sha256" in rec:
        assert cu.digest([len(p) for p in mine], flat) == rec["ref_sha256"]
        return
    assert [len(p) for p in mine] == list(rec["ref_path_sizes"]) and flat == list(rec["ref_path_nodes"])


def test_one_parametrised_case_per_golden_case_and_the_situations():
    text = [c["name"] for c in _MERGE.values() if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    t = GOLDEN["totals"]
    assert t["applications"] == sum(len(c["results"]) for c in CASES) == 4 * len(text) + len(DIRECT)
    for k in ("covered_late_start", "uncovered_ring", "blocked_start", "path_through_excluded_nodes", "path_ending_at_its_first_node",
              "reported_isolated_node", "dropped_isolated_node", "sum_above_32_bits", "reference_paths"):
        assert t[k] > 0, k
    assert t["max_path_rounds"] > 8 and t["max_cover_rounds"] > 8                     # both loops cross a batch


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_definition_and_device_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    want = [("a", DIRECT[case["name"][len("direct_"):]][4])] if case.get("direct") else [("b", 5000), ("b", 0), ("c", 5000), ("c", 0)]
    assert [(r["stage"], r["min_contig_len"]) for r in case["results"]] == want
    chain_nodes = {}
    for r in case["results"]:
        edges, order, n_ids, lengths = stages[r["stage"]]
        exclude, min_len = exclude_of(case, r), r["min_contig_len"]
        check_input(edges, order, lengths, exclude, r)
        assert r["n_ids"] == n_ids
        if not case.get("direct"):                                                    # X = the chain nodes of the stage before
            if r["stage"] not in chain_nodes:
                bc = bu.scheme(edges, order, 1, su.scheme(edges, order))
                chain_nodes[r["stage"]] = sorted(int(n) for n, c in zip(order, bc["node_chain"].tolist()) if c != bu.NONE)
            assert list(exclude) == chain_nodes[r["stage"]]
        sync, plain = ct.scheme(edges, order, lengths, exclude, min_len), ct.definition(edges, order, lengths, exclude, min_len)
        rank = {int(n): i for i, n in enumerate(order)}
        for res in (sync, plain):
            ct.check_against_record(res, r, edges)
            check_reference(res, edges, r)
            paths = res["c_first_edge"] != ct.NONE
            keys = [(rank[f], e) for f, e in zip(res["c_first"][paths].tolist(), res["c_first_edge"][paths].tolist())]
            assert keys == sorted(keys) and not paths[int(paths.sum()):].any()         # the numbering of the contract
            iso = [rank[f] for f in res["c_first"][~paths].tolist()]
            assert iso == sorted(iso)
            assert all(x >= min_len for x in res["c_length"].tolist())
        st = sync["stats"]
        assert {k: st[k] for k in ct.SCHEME_KEYS} == {k: r[k] for k in ct.SCHEME_KEYS}
        path_bound, cover_bound = ct.round_bounds(st)
        assert st["n_path_rounds"] <= path_bound and st["n_cover_rounds"] <= cover_bound
        assert st["n_covered_edges"] + st["n_uncovered_edges"] == st["n_edges"]
        assert st["n_contigs"] == st["n_paths"] - st["n_short_paths"] + st["n_isolated"] - st["n_short_isolated"]
        # layout.Contigs on the same arrays
        dev = as_device(sync, order, edges)
        assert len(dev) == st["n_contigs"]
        uv = cu.uv_of(edges)
        for j in range(min(len(dev), 50)):
            path = dev.path_of(j)
            assert path == ct.path_of(sync, edges, j) and len(path) == sync["c_nodes"][j]
            assert path[0] == sync["c_first"][j] and path[-1] == sync["c_last"][j]
            idx = dev.edges_of(j).tolist()
            assert [tuple(uv[e]) for e in idx] == list(zip(path, path[1:]))
            assert (idx[0] == sync["c_first_edge"][j]) if idx else (sync["c_first_edge"][j] == ct.NONE)
            w = np.asarray(edges, np.int64).reshape(-1, 4)[idx, 2].sum() if idx else 0
            assert int(w) + lengths[path[-1]] == sync["c_length"][j]


def test_the_shapes_the_direct_cases_are_about():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    table = lambda name: list(zip(by[name]["a_c_first"], by[name]["a_c_last"], by[name]["a_c_nodes"], by[name]["a_c_length"]))   # noqa: E731
    for tag in ("identity", "reversed", "scrambled", "zigzag"):
        r = by["path_1025_" + tag]
        assert (r["n_contigs"], r["n_paths"], r["max_path_nodes"], r["n_path_rounds"], r["n_cover_rounds"]) == (1, 1, 1025, 11, 1)
        assert r["a_c_first"] == [0] and r["a_c_last"] == [2048]
    big = 2**31 - 1
    assert table("weight_sum_above_2_to_32") == [(0, 6, 4, 3 * big - 3 + 106)] and 3 * big - 3 + 106 >= 2**32
    assert by["weight_sum_below_a_64_bit_minimum"]["n_short_paths"] == 1 and by["weight_sum_below_a_64_bit_minimum"]["n_contigs"] == 0
    for m in (40, 1025):                                                              # nothing covered, the loops end at once
        r = by["ring_%d" % m]
        assert (r["n_uncovered_edges"], r["n_root_starts"], r["n_late_starts"], r["n_path_rounds"], r["n_cover_rounds"]) == (m, 0, 0, 1, 1)
    assert sorted(table("lasso"))[0][:3] == (0, 8, 5) and sorted(table("lasso"))[1][:3] == (8, 8, 9)   # the ring's path ends where it began
    r = by["ring_with_a_spur_out"]
    assert (r["n_late_starts"], r["n_paths"], r["n_uncovered_edges"]) == (2, 0, 9)
    r = by["comb_300"]
    assert (r["n_root_starts"], r["n_late_starts"], r["n_paths"], r["max_cover_depth"], r["n_cover_rounds"]) == (2, 598, 600, 299, 10)
    r = by["binary_out_tree_depth_10"]
    assert (r["n_paths"], r["max_cover_depth"], r["n_cover_rounds"]) == (2046, 9, 5)
    r = by["blocked_root_start_with_a_tree_behind"]
    assert (r["n_blocked"], r["n_covered_edges"], r["n_contigs"]) == (1, 0, 0)
    r = by["blocked_late_start_beside_an_open_sibling"]
    assert (r["n_blocked"], r["n_covered_edges"], r["n_uncovered_edges"]) == (1, 3, 3)
    assert [t[:3] for t in table("blocked_late_start_beside_an_open_sibling")] == [(0, 2, 2), (2, 12, 3)]
    assert [t[:3] for t in table("path_through_a_stretch_of_excluded_nodes")] == [(0, 14, 8)]
    assert by["every_node_excluded"]["n_covered_edges"] == 0
    assert sorted(t[:3] for t in table("self_loop_as_head_edge")) == [(0, 2, 2), (2, 2, 2), (2, 6, 3)]
    assert [t[:3] for t in table("self_loop_on_an_in_degree_1_node")] == [(0, 0, 1)] and by["self_loop_on_an_in_degree_1_node"]["n_uncovered_edges"] == 3
    assert sorted(t[:3] for t in table("two_cycle_entered_from_outside")) == [(0, 2, 2), (2, 2, 3)]
    assert table("isolated_nodes_at_and_below_the_minimum") == [(8, 8, 1, 61), (4, 4, 1, 60)]       # by rank; 59 and the path of 15 dropped
    assert by["isolated_nodes_at_and_below_the_minimum"]["n_short_isolated"] == 1 and by["isolated_nodes_at_and_below_the_minimum"]["n_short_paths"] == 1
    assert by["minimum_0_reports_everything_covered"]["n_contigs"] == 2                 # the length -5 is below 0
    assert by["negative_length_is_below_every_minimum"]["n_contigs"] == 0
    r = by["pairs_2050_scrambled"]
    assert (r["n_paths"], r["n_contigs"]) == (2050, 2033)
    assert by["empty"]["n_nodes"] == 0 and by["empty"]["n_contigs"] == 0


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    for f in (ct.definition, ct.scheme):
        with pytest.raises(ValueError):
            f([(0, 2, 1), (2, 4, 1)], [0, 2], {0: 1, 2: 1})
