"""tests/merge_utils.py -- the plain statement of po_layout_merge and the scheme the kernels use (pointer jumping, sort of
the heads' ranks) -- against every application of tests/golden/merge_cases.npz, which the reference's own
merge_unambiguous_paths produced (tests/golden/make_merge_golden.py), and the GFA2 lines built from the tables against
the digests of the file the reference's gfa2_write_graph wrote."""
import numpy as np
import pytest

import diamond_utils as du
import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu
from test_diamond_oracle import case_stage1 as diamond_case_stage1, reduce_flags

GOLDEN = mu.load_golden()
CASES = GOLDEN["cases"]
TEXT_CASES = [c for c in CASES if not c.get("direct")]
_TEXT, _INPUT = {}, {}


def case_stage1(c):
    """(rows, node lengths, stage-1 edges in insertion order) of a text case; the ring and lasso cases on their own."""
    if c.get("synth", {}).get("kind") not in mu.SYNTH:
        return diamond_case_stage1(c)
    if c["name"] not in _TEXT:
        import layout_utils as lu
        from oracle import layout_oracle as lo
        from phasm_amd.io import gfa
        _, lengths, rows = gfa.read_gfa2_rows(mu.case_text(c).splitlines(True))
        L = lu.node_lengths(lengths)
        got = lo.layout_sequential(rows, L, **c["params"])["edges"]
        _TEXT[c["name"]] = (rows, L, np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4))
    return _TEXT[c["name"]]


def node_lengths(c):
    if c.get("direct"):
        return [mu.direct_length(n) for n in range(c["results"][0]["n_ids"])]
    return [int(x) for x in case_stage1(c)[1]]


def node_names(c):
    from phasm_amd.io import gfa
    names, _, _ = gfa.read_gfa2_rows(mu.case_text(c).splitlines(True))
    return [n + s for n in names for s in "+-"]


def input_edges(c, r):
    """The edges one recorded application started from, ordered by (u, v) as the golden's flags are (computed once)."""
    key = (c["name"], r["stage"])
    if key not in _INPUT:
        if c.get("direct"):
            e = np.asarray(c["edges"], dtype=np.int64).reshape(-1, 4)
        else:
            e = case_stage1(c)[2]
            if r["stage"] == "b":
                _, e, left, _ = du.clean_chain(e, c["order"], reduce_flags=reduce_flags(c, e))
                assert left == r["order_before"]
        e = e[tu.by_uv(e)]
        assert len(e) == r["n_in"]
        _INPUT[key] = e
    return _INPUT[key]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_device_scheme_equal_the_reference(case):
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["a", "b"])
    L = node_lengths(case)
    for r in case["results"]:
        e = input_edges(case, r)
        res = mu.merge_paths(e, r["order_before"], L, r["n_ids"])
        mu.check_against_record(res, r, e)
        assert r["n_edges_out"] == r["n_edges_in"] - (r["n_nodes_merged"] - r["n_merged"])
        for seed in (4, 5):                  # heads in two scrambled orders (the generator used two others)
            rr = mu.merge_paths_rounds(e, r["order_before"], L, r["n_ids"], seed)
            mu.check_against_record(rr, r, e)
            assert rr["edges"].tolist() == res["edges"].tolist()
            n = max(r["n_nodes"], 1)
            assert rr["stats"]["n_rounds"] <= r["rounds"] <= int(np.ceil(np.log2(n))) + 1
            assert (rr["stats"]["n_rounds"] > 0) == (r["n_merged"] > 0)
        # the numbering follows the node order, nothing else does
        rev = mu.merge_paths(e, r["order_before"][::-1], L, r["n_ids"])
        assert np.array_equal(rev["flags"], res["flags"]) and sorted(rev["lengths"].tolist()) == sorted(res["lengths"].tolist())


@pytest.mark.parametrize("case", TEXT_CASES, ids=[c["name"] for c in TEXT_CASES])
def test_the_lines_built_from_the_tables_equal_the_file_of_the_reference(case):
    r = case["results"][1]
    e = input_edges(case, r)
    L = node_lengths(case)
    res = mu.merge_paths(e, r["order_before"], L, r["n_ids"])
    head, e_lines = mu.gfa_lines(res, node_names(case), L, r["n_ids"])
    assert len(head) == r["n_hsf_lines"] and mu.lines_digest(head) == r["hsf_sha256"]
    assert mu.lines_digest(sorted(e_lines)) == r["e_sorted_sha256"]
    assert sum(l[0] == "F" for l in head) == r["n_nodes_merged"]


def test_every_branch_is_taken():
    totals = GOLDEN["branch_totals"]
    assert set(mu.BRANCHES) <= set(totals)
    for k in mu.BRANCHES:
        assert totals[k] > 0, k
    assert totals["max_rounds"] >= 10
    # the reference alone met every condition but the pure cycles, which the ring cases bring
    alone = GOLDEN["reference_alone"]
    assert all(alone[k] > 0 for k in mu.BRANCHES if k != "cycle_nodes")
    assert GOLDEN["text_totals"]["cycle_nodes"] > alone["cycle_nodes"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("name,merged,nodes,cycle,self_loops", [
    ("path_2", 1, 2, 0, 0), ("path_3", 1, 3, 0, 0), ("path_64", 1, 64, 0, 0), ("path_65_scrambled", 1, 65, 0, 0),
    ("path_1025_reversed", 1, 1025, 0, 0), ("path_4097_reversed", 1, 4097, 0, 0),
    ("cycle_1", 0, 0, 1, 0), ("cycle_2", 0, 0, 2, 0), ("cycle_3", 0, 0, 3, 0), ("cycle_64", 0, 0, 64, 0), ("cycle_65", 0, 0, 65, 0),
    ("lasso_tail_first", 2, 8, 0, 1), ("lasso_ring_reversed_first", 2, 8, 0, 1), ("lasso_exit_into_a_path", 3, 11, 0, 1),
    ("two_cycle_with_tail", 1, 2, 0, 1), ("path_into_self_loop", 1, 2, 0, 0), ("fork", 2, 5, 0, 0),
    ("pairs_64_heads_against_ids", 64, 128, 0, 0), ("pairs_65_heads_against_ids", 65, 130, 0, 0),
    ("pairs_257_heads_against_ids", 257, 514, 0, 0), ("path_and_its_mirror_interleaved", 2, 8, 0, 0),
    ("empty", 0, 0, 0, 0), ("nodes_without_edges", 0, 0, 0, 0), ("overflow", 1, 4, 0, 0)])
def test_direct_shapes(name, merged, nodes, cycle, self_loops):
    r = by_name("direct_" + name)["results"][0]
    assert (r["n_merged"], r["n_nodes_merged"], r["n_cycle_nodes"], r["n_self_loops"]) == (merged, nodes, cycle, self_loops)


def test_numbering_by_rank_not_by_index():
    c = by_name("direct_pairs_65_heads_against_ids")
    r = c["results"][0]
    heads = r["members"][r["offsets"][:-1]].tolist()
    assert heads == sorted(heads, reverse=True) and heads == [n for n in r["order_before"] if n in set(heads)]


def test_the_overflow_case_overflows():
    r = by_name("direct_overflow")["results"][0]
    assert r["n_overflow"] == 2 and int(r["prefix"].sum()) == 3 * 2**30


def test_a_lasso_keeps_the_edge_back_to_its_head_as_a_self_loop():
    c = by_name("direct_lasso_tail_first")
    r = c["results"][0]
    res = mu.merge_paths(input_edges(c, r), r["order_before"], node_lengths(c), r["n_ids"])
    loops = [x for x in res["edges"].tolist() if x[0] == x[1]]
    assert len(loops) == 1 and loops[0][0] >= r["n_ids"]
    k = loops[0][0] - r["n_ids"]
    last_to_head = next(x for x in c["edges"] if x[0] == 10 and x[1] == 0)
    assert loops[0][2] == last_to_head[2] + int(res["prefix"][res["offsets"][k]:res["offsets"][k + 1]].sum())


@pytest.mark.parametrize("name", ["union_21_1", "selfish_2", "reduced_line_101", "lasso_12_8", "ring_3"])
def test_the_library_writer_writes_the_file_of_the_reference(name):
    """phasm_amd.layout.write_merged_graph (what ``layout-edges --merge`` calls) on the statement's tables: no GPU."""
    import io
    from phasm_amd import _lib, layout
    case = by_name(name)
    r = case["results"][1]
    e, L = input_edges(case, r), node_lengths(case)
    res = mu.merge_paths(e, r["order_before"], L, r["n_ids"])
    edges = np.zeros(len(res["edges"]), dtype=_lib.EDGE_DTYPE)
    for k, key in enumerate(("u", "v", "weight", "overlap_len")):
        edges[key] = res["edges"][:, k]
    g = layout.AssemblyEdges(edges, np.zeros(r["n_ids"] // 2, bool), node_names(case), {},
                             merged_paths=(res["offsets"], res["members"], res["prefix"], res["lengths"]),
                             node_order=np.asarray(res["order"]), node_lengths=np.asarray(L))
    f = io.StringIO()
    assert layout.write_merged_graph(f, g) == r["n_edges_out"]
    lines = f.getvalue().splitlines(True)
    head = lines[:r["n_hsf_lines"]]
    assert mu.lines_digest(head) == r["hsf_sha256"] and mu.lines_digest(sorted(lines[len(head):])) == r["e_sorted_sha256"]
    assert g.node_name(r["n_ids"]) == "merged0+" and g.node_name(0) == node_names(case)[0]
    if r["n_merged"]:
        assert g.node_length(r["n_ids"]) == int(res["lengths"][0]) and g.edge_tuples()[0][0] == g.node_name(edges["u"][0])
