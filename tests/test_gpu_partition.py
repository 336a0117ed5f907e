"""Strongly connected components and the superbubble partition on the device (po_layout_partition,
layout.strongly_connected_components, layout.superbubble_partitions, ``chain-components --partitions``) against
tests/golden/partition_cases.npz: the reference's partition_graph, unmodified, on the reference's graphs at two stages and on
the direct cases.  Exact integers throughout.  The one direct case with merged-node ids cannot go through
po_graph_from_edges (its ends are oriented reads by contract); merged ids reach the device in every stage-(c) application
here, and tests/test_partition_host_emulation.py runs the kernels on the case itself."""
import logging

import numpy as np
import pytest

import components_utils as cu
import partition_utils as pu
from phasm_amd import layout
from phasm_amd.io import gfa
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs
from test_gpu_components import FILE_CASES, merge_bytes, segments
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text
from test_partition_oracle import CASES, stage_inputs

pytestmark = pytest.mark.gpu

TEXT = [c for c in CASES if not c.get("direct")]
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1
ROUND_KEYS = ("n_trim_rounds", "n_forward_rounds", "n_backward_rounds")


def as_result(sccs):
    st = dict(sccs.stats)
    return {"node_scc": sccs.scc_of_node.astype(np.int64), "node_flags": sccs.node_flags.astype(np.int64),
            "edge_class": sccs.edge_class.astype(np.int64), "stats": st, **{k: sccs.table[k].astype(np.int64) for k in sccs.table.dtype.names}}


def check_partition(ov, res, rec, want_inputs=None):
    """One application on the graph result ``res`` against its record; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    sccs = layout.strongly_connected_components(ov, res)
    comps = layout.weakly_connected_components(ov, res)
    st = sccs.stats
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    got = as_result(sccs)
    parts = layout.superbubble_partitions(sccs, comps)
    pu.check_against_record(got, pu.device_partitions(parts, e), e, rec)              # the golden: the reference's sets
    want = pu.partition(e, order.tolist())                                           # the restatement, on the device's own edge order
    for k in pu.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    rank = np.zeros(int(order.max()) + 1 if len(order) else 0, np.int64)
    rank[order] = np.arange(len(order))
    assert sccs.scc_of_edge.tolist() == (want["node_scc"][rank[e[:, 0]]].tolist() if len(e) else [])
    assert all(p[-1].acyclic and not any(q.acyclic for q in p[:-1]) for p in parts) and len(parts) == len(comps)
    # the stats are consistent: class counts sum to the edges, rounds stay within the caps (no particular count is asserted)
    n = len(order)
    assert st["n_invalid"] == 0 and sum(st["n_class"]) == st["n_edges"] == len(e) and st["n_nodes"] == n
    assert st["n_sccs"] == st["n_singletons"] + st["n_nonsingleton_sccs"] == len(sccs) and st["n_trimmed"] <= st["n_singletons"]
    assert st["n_outer"] <= n and (st["n_outer"] > 0) == (n > 0)
    assert all(st[k] <= st["n_outer"] * (n + 2) for k in ROUND_KEYS) and st["n_trim_rounds"] >= st["n_outer"]
    rounds = sum(st[k] for k in ROUND_KEYS)
    assert -(-rounds // 8) <= st["n_batches"] <= rounds // 8 + 3 * st["n_outer"]
    if want_inputs is not None:
        w_edges, w_order, _ = want_inputs
        assert order.tolist() == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: %d iterations, rounds %d / %d / %d (synchronous %d / %d / %d), %d batches, %.3f ms" % (
        rec["stage"], st["n_outer"], st["n_trim_rounds"], st["n_forward_rounds"], st["n_backward_rounds"], rec["n_trim_rounds"],
        rec["n_forward_rounds"], rec["n_backward_rounds"], st["n_batches"], st["ms_total"]))
    return sccs.scc_of_node.tobytes() + sccs.node_flags.tobytes() + sccs.edge_class.tobytes() + sccs.table.tobytes()


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_partition_from_gfa_text_equals_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_b, rec_c = case["results"]
    final = cleaned(ov, edges_res)
    merge_before = merge_bytes(ov, final)
    check_partition(ov, final, rec_b, stages["b"])                         # (b) after the cleaning chain
    assert merge_bytes(ov, final) == merge_before                          # a merge after the call gives the same bytes
    merged = ov.layout_merge(final)
    check_partition(ov, merged, rec_c, stages["c"])                        # (c) the merged graph: node ids >= the reads
    assert len(ov) == rec_c["n_ids"]
    for r in (merged, final, edges_res):
        r.free()
    ov.close()


def direct_graph(case):
    uv, order, n_ids = stage_inputs(case)["a"]
    ov = segments(n_ids)
    e = np.concatenate([uv, np.full((len(uv), 1), 100), np.full((len(uv), 1), 17)], axis=1).astype(np.int64)
    return ov, ov.graph_from_edges(e, order), (uv, order, n_ids)


@pytest.mark.parametrize("case", DIRECT, ids=[c["name"] for c in DIRECT])
def test_direct_cases_through_graph_from_edges(case):
    ov, g, inputs = direct_graph(case)
    assert len(g) == len(inputs[0]) and g.node_order().tolist() == list(inputs[1])
    check_partition(ov, g, case["results"][0], inputs)
    g.free()
    ov.close()


def test_three_calls_and_a_fresh_handle_give_identical_bytes(tmp_path):
    case = next(c for c in TEXT if c["name"] == "selfish_1")
    seen = []
    for calls in (3, 1):
        ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
        final = cleaned(ov, edges_res)
        merged = ov.layout_merge(final)
        for _ in range(calls):
            seen.append(check_partition(ov, final, case["results"][0]) + check_partition(ov, merged, case["results"][1]))
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 4 and all(s == seen[0] for s in seen)
    rnd = next(c for c in DIRECT if c["name"] == "direct_random_200_300_seed1")
    seen = []
    for calls in (3, 1):
        ov, g, _ = direct_graph(rnd)
        seen += [check_partition(ov, g, rnd["results"][0]) for _ in range(calls)]
        g.free()
        ov.close()
    assert all(s == seen[0] for s in seen)


TURN_NAMES = ("direct_three_cycle_with_tails", "direct_ring_1025_scrambled", "direct_random_200_300_seed1")   # small, large, small


def test_components_and_partition_take_turns_in_the_rank_workspaces_of_one_handle():
    """Both calls rank the graph in the same buffers of the handle: on one handle they alternate, twice each, on a few
    nodes, then 1 025, then 200, so every call finds what a call of the other stage -- and, behind the large graph, of a
    larger graph -- left there.  Every call's arrays are the restatements', and its bytes those of the same call on a
    handle that has run nothing else."""
    inputs = [stage_inputs(next(c for c in DIRECT if c["name"] == name))["a"] for name in TURN_NAMES]
    n_ids = max(i[2] for i in inputs)
    assert [len(i[1]) for i in inputs] == [5, 1025, 200]

    def graph(ov, uv, order):
        return ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 1), 100), np.full((len(uv), 1), 17)], axis=1).astype(np.int64), order)

    def components(ov, g):
        nodes, edges, table = ov.layout_components(g)
        return {"node_component": nodes, "edge_component": edges, **{k: table[k] for k in table.dtype.names}}

    def partition(ov, g):
        nodes, flags, classes, table = ov.layout_partition(g)
        return {"node_scc": nodes, "node_flags": flags, "edge_class": classes, **{k: table[k] for k in table.dtype.names}}

    def fresh(call, uv, order):
        ov = segments(n_ids)
        g = graph(ov, uv, order)
        out = call(ov, g)
        g.free()
        ov.close()
        return out

    ov = segments(n_ids)
    for uv, order, _ in inputs:
        g = graph(ov, uv, order)
        e = edge_array(g.rows())
        want = {components: cu.weak_components(e[:, :2], list(order)), partition: pu.partition(e, list(order))}
        alone = {call: fresh(call, uv, order) for call in (components, partition)}
        for call in (components, partition, components, partition):
            got = call(ov, g)
            assert set(got) == set(alone[call]) and len(got) >= 5
            for k, a in got.items():
                assert a.tolist() == np.asarray(want[call][k]).tolist(), (call.__name__, k)
                assert a.dtype == alone[call][k].dtype and a.tobytes() == alone[call][k].tobytes(), (call.__name__, k)
        g.free()
    ov.close()


def expected_lines(parts):
    return ["Partition with %d nodes with in-degree 0, %d nodes with out-degree 0, acyclic: %s" % (p["num_sources"], p["num_sinks"], p["acyclic"])
            for p in parts]


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_file_route_equals_the_reference(name, tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in TEXT if c["name"] == name)
    rec = case["results"][1]
    text = component_stage_inputs(next(c for c in COMPONENT_CASES if c["name"] == name))["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    g = layout.chain_components(str(p), partitions=True)
    plain = layout.chain_components(str(p))
    assert plain.partitions is None and plain.sccs is None
    assert plain.components.component_of_node.tobytes() == g.components.component_of_node.tobytes()
    # the file numbers its nodes by its own S lines: the stage-(c) graph under the ids of the golden (read i of the file
    # is read names[i]; a merged segment k is node n_ids + k)
    graph = g.graph
    e_c, order_c, n_ids = stage_inputs(case)["c"]
    assert len(graph.node_order) == len(order_c) == rec["n_nodes"] and len(graph.edges) == rec["n_edges"]
    want = pu.partition(graph.edges, graph.node_order)
    weak = cu.weak_components(graph.edges, graph.node_order)
    want_parts = pu.reference_partitions(want, weak, graph.edges, graph.node_order)
    got_parts = pu.device_partitions(g.partitions, graph.edges)
    assert got_parts == want_parts
    # ... and has the reference's partitions of the stage-(c) graph: the same counts per partition, whatever the numbering
    shape = lambda parts: sorted((p["acyclic"], len(p["nodes"]), len(p["edges"]), p["num_sources"], p["num_sinks"]) for p in parts)   # noqa: E731
    assert shape(got_parts) == sorted(zip(map(bool, rec["p_acyclic"]), rec["p_n_nodes"], rec["p_n_edges"], rec["p_sources"], rec["p_sinks"])) \
        if "p_acyclic" in rec else len(got_parts) == rec["n_partitions"]
    assert g.sccs.stats["n_sccs"] == rec["n_sccs"] and g.sccs.stats["n_class"] == rec["n_class"]
    # the command: with the flag one line per partition in the reference's wording; without it today's output and files
    outs = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["chain-components", str(p), "-o", str(out), "-f", "gfa2,graphml"] + (["--partitions"] if flag else [])) == 0
        lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Partition with")]
        assert lines == (expected_lines(want_parts) if flag else [])
        outs[flag] = ({f.name: f.read_bytes() for f in sorted(out.iterdir())},
                      [r.getMessage() for r in caplog.records if not r.getMessage().startswith("Partition with")])
    assert outs[True] == outs[False] and len(outs[False][0]) == 2 * len(g.components)
    assert gfa.read_graph_gfa(text.splitlines(True)).edges.tolist() == graph.edges.tolist()


def test_an_empty_graph_and_null_outputs():
    import ctypes
    from phasm_amd import _lib
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    nodes, flags, classes, table = ov.layout_partition(g)
    assert len(nodes) == len(flags) == len(classes) == len(table) == 0 and ov.partition_stats()["n_sccs"] == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 0, 1, 1], [2, 4, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    assert _lib.load().po_layout_partition(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 3
    g.free()
    ov.close()
