"""tests/components_utils.py -- the plain statement of po_layout_components and the device's scheme run synchronously --
against every application of tests/golden/components_cases.npz (tests/golden/make_components_golden.py: networkx on the
reference's graphs at three stages), the reader of phasm_amd/io/gfa.py against the reference's reconstruction of the
graph files, and the component writers of phasm_amd/layout.py against the digests of what the reference's writers wrote."""
import numpy as np
import pytest

import components_utils as cu
import merge_utils as mu
from phasm_amd import layout
from phasm_amd.io import gfa
from test_merge_oracle import CASES as MERGE_CASES, input_edges, node_lengths, node_names

GOLDEN = cu.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids) for name, order, edges, n_ids in cu.direct_inputs()}
_MERGE = {c["name"]: c for c in MERGE_CASES}
_STAGES = {}


def stage_inputs(case):
    """{stage: (edges [n, >=2], node order, n_ids)} of a golden case, computed once: a direct case's own, or the graphs of
    the text case at (a) stage 1, (b) after the cleaning chain, (c) after the merge, rebuilt from the inputs that
    tests/golden/merge_cases.npz pins; with them for a text case "file": the text of the graph file the reference wrote."""
    name = case["name"]
    if name in _STAGES:
        return _STAGES[name]
    if case.get("direct"):
        order, edges, _ = DIRECT[name[len("direct_"):]]
        out = {"a": (np.asarray(edges, dtype=np.int64).reshape(-1, 2), list(order), case["results"][0]["n_ids"])}
    else:
        mc = _MERGE[name]
        ra, rb = mc["results"]
        L, n_ids = node_lengths(mc), ra["n_ids"]
        e_b = input_edges(mc, rb)
        merged = mu.merge_paths(e_b, rb["order_before"], L, n_ids)
        out = {"a": (input_edges(mc, ra), ra["order_before"], n_ids), "b": (e_b, rb["order_before"], n_ids),
               "c": (merged["edges"], merged["order"], n_ids)}
        names = dict(enumerate(node_names(mc)))
        head, e_lines = mu.gfa_lines(merged, names, L, n_ids)
        lines = head + [e_lines[i] for i in case["file"]["e_perm"]]
        assert mu.lines_digest(lines) == case["file"]["text_sha256"], "the graph file differs from the one the reference wrote"
        out["file"] = "".join(lines)
    _STAGES[name] = out
    return out


def check_input(edges, order, rec):
    e = cu.uv_of(edges)
    assert cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))]) == rec["in_sha256"], "the input differs from the generator's"


def test_one_parametrised_case_per_golden_case():
    assert len(CASES) == len(set(c["name"] for c in CASES)) == len(_MERGE) - sum(1 for c in MERGE_CASES if c.get("direct")) + len(DIRECT)
    assert GOLDEN["totals"]["hand_raises"] == 0 and len(GOLDEN["hand_files"]) == len(cu.HAND_FILES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_device_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["a", "b", "c"])
    for r in case["results"]:
        edges, order, n_ids = stages[r["stage"]]
        check_input(edges, order, r)
        assert r["n_ids"] == n_ids
        plain, sync = cu.weak_components(edges, order), cu.components_rounds(edges, order)
        for res in (plain, sync):
            cu.check_against_record(res, r)
            rank = {n: i for i, n in enumerate(order)}
            assert res["edge_component"].tolist() == [int(res["node_component"][rank[int(u)]]) for u in cu.uv_of(edges)[:, 0]]
            # the numbering: component i starts at the i-th lowest-ranked first node
            assert [rank[int(f)] for f in res["first_node"]] == sorted(rank[int(f)] for f in res["first_node"])
        assert sync["stats"]["rounds"] == r["rounds"] <= len(order) + 2


def file_route(text, rec):
    graph = gfa.read_graph_gfa(text.splitlines(True))
    e = graph.edges
    assert graph.node_order == rec["file_order"]
    assert cu.digest(e[np.lexsort((e[:, 1], e[:, 0]))]) == rec["file_edges_sha256"]
    comps = cu.weak_components(e, graph.node_order)
    cu.check_against_record(comps, rec)
    written = []
    for i in range(rec["n_components"]):
        nodes = [n for n, c in zip(graph.node_order, comps["node_component"].tolist()) if c == i]
        mine = e[np.flatnonzero(comps["edge_component"] == i)]
        written.append((layout.component_gfa2_lines(graph, nodes, mine), layout.component_gfa1_lines(graph, nodes, mine)))
    assert cu.writers_digest(written) == rec["writers_sha256"]
    return graph


@pytest.mark.parametrize("case", [c for c in CASES if not c.get("direct")], ids=[c["name"] for c in CASES if not c.get("direct")])
def test_reader_and_writers_equal_the_reference_on_the_graph_file(case):
    assert "raises" not in case["file"]
    graph = file_route(stage_inputs(case)["file"], case["file"])
    # the file's graph is the stage-(c) graph under the file's own numbering
    c = case["results"][2]
    assert (len(graph.node_order), len(graph.edges)) == (c["n_nodes"], c["n_edges"])
    assert case["file"]["n_components"] == c["n_components"]


@pytest.mark.parametrize("rec", GOLDEN["hand_files"], ids=[r["name"] for r in GOLDEN["hand_files"]])
def test_reader_rules_on_the_hand_written_files(rec):
    graph = file_route(cu.HAND_FILES[rec["name"]], rec)
    if rec["name"] == "duplicated_edge_line":      # the second line's attributes at the first line's place
        assert graph.edges.tolist() == [[0, 2, 40, 65], [2, 4, 50, 40]]
    if rec["name"] == "dollar_positions":
        assert graph.edges.tolist() == [[0, 2, 40, 60], [3, 1, 30, 60]]   # overlap_len = max of the two ranges
    if rec["name"] == "segments_without_edges_between":
        assert graph.node_order == [6, 2, 0, 4, 8]
    if rec["name"] == "minus_strand_only":
        assert graph.node_order == [3, 1, 4]
    if rec["name"] == "merged_segment_without_edges":
        assert graph.node_order == [0, 4, 2] and graph.fragments == {1: (["x+", "y-"], [60])}
    if rec["name"] == "merged_segment_fragments_out_of_order":
        assert graph.fragments == {0: (["x+", "y-"], [60])} and graph.lengths.tolist() == [150, 101]
        with pytest.raises(KeyError):
            gfa.read_graph_gfa(["S\tm\t9\t*\n", "F\tm\tx+\t0\t9\t0\t9\t*\n", "S\ta\t5\t*\n", "E\t*\tm-\ta+\t1\t9\t0\t4\t*\n"])
