"""The bubble chains on the device (po_layout_bubblechains, layout.bubble_chains, ``chain-components --bubblechains``) against
tests/golden/bubblechain_cases.npz: the reference's build_bubblechains, unmodified, on the qualifying components of the
reference's graphs at two stages and of the direct cases.  Exact integers throughout.  The one direct case with merged-node
ids cannot go through po_graph_from_edges (its ends are oriented reads by contract); merged ids reach the device in every
stage-(c) application here, and tests/test_bubblechains_host_emulation.py runs the kernels on the case itself."""
import ctypes
import logging

import numpy as np
import pytest

import bubblechain_utils as bu
import components_utils as cu
import partition_utils as pu
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_bubblechains_oracle import CASES, check_reference, stage_inputs
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs
from test_gpu_components import FILE_CASES, merge_bytes, segments
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text

pytestmark = pytest.mark.gpu

TEXT_NAMES = ["selfish_1", "tangle_3", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
             [c["name"] for c in CASES if c["name"].startswith("union_")]
TEXT = [c for c in CASES if c["name"] in TEXT_NAMES]
assert len(TEXT) == len(TEXT_NAMES) > 6
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1


def as_result(bc):
    none = lambda a: np.where(a == _lib.NO_NODE, bu.NONE, a.astype(np.int64))   # noqa: E731
    t = bc.table
    return {"node_chain": none(bc.node_chain), "node_bubble": none(bc.node_bubble), "edge_chain": none(bc.edge_chain),
            "c_first": t["first_entrance"].astype(np.int64), "c_last": t["last_exit"].astype(np.int64),
            "c_bubbles": t["n_bubbles"].astype(np.int64), "c_nodes": t["n_nodes"].astype(np.int64), "c_edges": t["n_edges"].astype(np.int64),
            "stats": dict(bc.stats)}


def call_bytes(bc):
    return bc.node_chain.tobytes() + bc.node_bubble.tobytes() + bc.edge_chain.tobytes() + bc.table.tobytes()


def check_bubblechains(ov, res, rec, want_inputs=None):
    """One application on the graph result ``res`` against its record; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    min_nodes = rec["min_nodes"]
    bc = layout.bubble_chains(ov, res, min_nodes)
    st = bc.stats
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    got = as_result(bc)
    bu.check_against_record(got, rec, e)                                                 # the golden: the contract's arrays
    check_reference(got, e, order.tolist(), rec)                                         # ... and the reference's chains
    sb = su.scheme(e, order.tolist())
    want = bu.scheme(e, order.tolist(), min_nodes, sb)                                   # the restatement, on the device's own edge order
    for k in bu.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert bc.node_chain.dtype == bc.node_bubble.dtype == bc.edge_chain.dtype == np.uint32 and bc.table.dtype == _lib.BUBBLECHAIN_DTYPE
    for j in range(min(len(bc), 20)):
        assert bc.nodes_of(j).tolist() == bu.nodes_of(want, order.tolist(), j) and len(bc.edges_of(j)) == want["c_edges"][j]
        assert bc.bubbles_of(j) == bu.bubbles_of(want, order.tolist(), sb, j)
    # the stats: the contract's counts, rounds within the logarithmic bounds, batches within what the loops allow
    n = len(order)
    assert st["n_invalid"] == 0 and st["n_nodes"] == n and st["n_edges"] == len(e)
    assert {k: st[k] for k in bu.STAT_KEYS} == {k: rec[k] for k in bu.STAT_KEYS}
    nest_bound, chain_bound = bu.round_bounds({"n_levels_forward": rec["n_levels_forward"], "max_chain_bubbles": st["max_chain_bubbles"]})
    assert st["n_nest_rounds"] <= rec["n_nest_rounds"] <= nest_bound and st["n_chain_rounds"] == rec["n_chain_rounds"] <= chain_bound
    if n:
        assert (st["n_nest_rounds"] > 0) == (st["n_top"] > 0 and st["n_bubbles"] > st["n_top"]) and (st["n_chain_rounds"] > 0) == (st["n_top"] > 0)
        assert st["n_batches"] >= -(-(st["n_nest_rounds"] + st["n_chain_rounds"]) // 8)
    if want_inputs is not None:
        w_edges, w_order, _ = want_inputs
        assert order.tolist() == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: %d chains (%d short), longest %d, rounds %d + %d, %d batches, %.3f ms (superbubbles %.3f, chains %.3f, label %.3f)" % (
        rec["stage"], st["n_chains"], st["n_short"], st["max_chain_bubbles"], st["n_nest_rounds"], st["n_chain_rounds"], st["n_batches"],
        st["ms_total"], st["ms_superbubbles"], st["ms_chains"], st["ms_label"]))
    return call_bytes(bc)


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_bubblechains_from_gfa_text_equal_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_b, rec_c = case["results"]
    final = cleaned(ov, edges_res)
    merge_before = merge_bytes(ov, final)
    check_bubblechains(ov, final, rec_b, stages["b"])                      # (b) after the cleaning chain
    assert merge_bytes(ov, final) == merge_before                          # a merge after the call gives the same bytes
    merged = ov.layout_merge(final)
    check_bubblechains(ov, merged, rec_c, stages["c"])                     # (c) the merged graph: node ids >= the reads
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
    check_bubblechains(ov, g, case["results"][0], inputs)
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
            seen.append(check_bubblechains(ov, final, case["results"][0]) + check_bubblechains(ov, merged, case["results"][1]))
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 4 and all(s == seen[0] for s in seen)
    for name in ("direct_sb_random_dag_200_seed0", "direct_bc_nesting_depth_300", "direct_sb_path_1025_scrambled"):
        rnd = next(c for c in DIRECT if c["name"] == name)
        seen = []
        for calls in (3, 1):
            ov, g, _ = direct_graph(rnd)
            seen += [check_bubblechains(ov, g, rnd["results"][0]) for _ in range(calls)]
            g.free()
            ov.close()
        assert all(s == seen[0] for s in seen)


TURN_NAMES = ("direct_three_cycle_with_tails", "direct_sb_path_1025_scrambled", "direct_sb_random_digraph_200_seed1")   # small, large, small


def test_the_four_stages_take_turns_on_one_handle():
    """Components, partition, superbubbles and bubble chains rank the graph in the same buffers of the handle, and the last
    two run the superbubble stage in the same workspaces: on one handle they alternate, twice each, on a few nodes, then
    1 025, then 200, so every call finds what a call of another stage -- and, behind the large graph, of a larger graph --
    left there.  Every call's arrays are the restatements', and its bytes those of the same call on a handle that has run
    nothing else; the superbubbles in particular are unchanged by the bubble-chain calls around them."""
    inputs = [stage_inputs(next(c for c in DIRECT if c["name"] == name))["a"] for name in TURN_NAMES]
    n_ids = max(i[2] for i in inputs)
    assert [len(i[1]) for i in inputs] == [5, 1025, 200]

    def graph(ov, uv, order):
        return ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 1), 100), np.full((len(uv), 1), 17)], axis=1).astype(np.int64), order)

    none = lambda a: np.where(a == _lib.NO_NODE, su.NONE, a.astype(np.int64))   # noqa: E731

    def components(ov, g):
        nodes, edges, table = ov.layout_components(g)
        return {"node_component": nodes, "edge_component": edges, **{k: table[k] for k in table.dtype.names}}

    def partition(ov, g):
        nodes, flags, classes, table = ov.layout_partition(g)
        return {"node_scc": nodes, "node_flags": flags, "edge_class": classes, **{k: table[k] for k in table.dtype.names}}

    def superbubbles(ov, g):
        node_exit, node_inside, flags, table = ov.layout_superbubbles(g)
        return {"node_exit": none(node_exit), "node_inside": none(node_inside), "node_flags": flags, "b_entrance": table["entrance"],
                "b_exit": table["exit"], "b_inside": table["n_inside"], "b_nested": table["nested"]}

    def bubblechains(ov, g):
        node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains(g)
        return {"node_chain": none(node_chain), "node_bubble": none(node_bubble), "edge_chain": none(edge_chain),
                "c_first": table["first_entrance"], "c_last": table["last_exit"], "c_bubbles": table["n_bubbles"], "c_nodes": table["n_nodes"],
                "c_edges": table["n_edges"]}

    def fresh(call, uv, order):
        ov = segments(n_ids)
        g = graph(ov, uv, order)
        out = call(ov, g)
        g.free()
        ov.close()
        return out

    calls = (components, partition, superbubbles, bubblechains)
    ov = segments(n_ids)
    for uv, order, _ in inputs:
        g = graph(ov, uv, order)
        e = edge_array(g.rows())
        want = {components: cu.weak_components(e[:, :2], list(order)), partition: pu.partition(e, list(order)),
                superbubbles: su.scheme(e, list(order)), bubblechains: bu.scheme(e, list(order))}
        alone = {call: fresh(call, uv, order) for call in calls}
        for call in calls + calls[::-1] + (superbubbles, bubblechains, superbubbles):
            got = call(ov, g)
            assert set(got) == set(alone[call]) and len(got) >= 5
            for k, a in got.items():
                assert a.tolist() == np.asarray(want[call][k]).tolist(), (call.__name__, k)
                assert a.dtype == alone[call][k].dtype and a.tobytes() == alone[call][k].tobytes(), (call.__name__, k)
        g.free()
    ov.close()


def test_superbubble_bytes_and_stats_are_unchanged_by_an_interleaved_bubblechain_call():
    case = next(c for c in DIRECT if c["name"] == "direct_bc_nesting_depth_3_inside_a_chain_member")
    ov, g, _ = direct_graph(case)
    counts = lambda st: {k: v for k, v in st.items() if not k.startswith("ms_")}   # noqa: E731
    first = [a.tobytes() for a in ov.layout_superbubbles(g)]
    stats = counts(ov.superbubble_stats())
    ov.layout_bubblechains(g)
    assert counts(ov.superbubble_stats()) == stats                                    # the other call's stats are its own
    assert [a.tobytes() for a in ov.layout_superbubbles(g)] == first and counts(ov.superbubble_stats()) == stats
    g.free()
    ov.close()


def expected_files_and_lines(graph, want, weak):
    """{file name: text} of the chain files and the log lines of the chains, per component, from the restatement."""
    order = [int(n) for n in graph.node_order]
    comp_of = dict(zip(order, weak["node_component"].tolist()))
    per = [[] for _ in range(weak["stats"]["n_components"])]
    for c, first in enumerate(want["c_first"].tolist()):
        per[comp_of[first]].append(c)
    files, lines = {}, []
    for i, chains in enumerate(per):
        for j, c in enumerate(chains):
            nodes = bu.nodes_of(want, order, c)
            edges = graph.edges[np.flatnonzero(want["edge_chain"] == c)]
            lines.append("Found bubblechain #%d with %d nodes and %d edges" % (j, len(nodes), len(edges)))
            files["component%d.bubblechain%d.gfa" % (i, j)] = "".join(layout.component_gfa2_lines(graph, nodes, edges))
    return files, lines, per


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_file_route_with_and_without_the_flag(name, tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in CASES if c["name"] == name)
    rec = case["results"][1]
    text = component_stage_inputs(next(c for c in COMPONENT_CASES if c["name"] == name))["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    g = layout.chain_components(str(p), bubblechains=True)
    plain = layout.chain_components(str(p))
    assert plain.bubblechains is None and plain.component_chains is None and g.superbubbles is None
    assert plain.components.component_of_node.tobytes() == g.components.component_of_node.tobytes()
    # the file numbers its nodes by its own S lines: the stage-(c) graph under other ids than the golden's.  The arrays are
    # the restatement's on the file's own graph; the counts are the golden's, whatever the numbering
    graph = g.graph
    order = [int(n) for n in graph.node_order]
    assert len(order) == rec["n_nodes"] and len(graph.edges) == rec["n_edges"]
    want = bu.scheme(graph.edges, order)
    got = as_result(g.bubblechains)
    for k in bu.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: g.bubblechains.stats[k] for k in bu.STAT_KEYS} == {k: rec[k] for k in bu.STAT_KEYS}
    weak = cu.weak_components(graph.edges, order)
    files, lines, per = expected_files_and_lines(graph, want, weak)
    assert g.component_chains == per
    # the command: with the flag the chain files, their lines and the node attribute; without it today's output and files
    outs = {}
    mine = lambda m: m.startswith("Found bubblechain")   # noqa: E731
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["chain-components", str(p), "-o", str(out), "-f", "gfa2,graphml"] + (["--bubblechains"] if flag else [])) == 0
        said = [r.getMessage() for r in caplog.records]
        assert [m for m in said if mine(m)] == (lines if flag else [])
        outs[flag] = ({f.name: f.read_text() for f in sorted(out.iterdir())}, [m for m in said if not mine(m)])
    assert outs[True][1] == outs[False][1] and len(outs[False][0]) == 2 * len(g.components)
    assert not any("bubblechain" in n or "bubblechain" in t for n, t in outs[False][0].items())
    with_flag, without = outs[True][0], outs[False][0]
    assert {n: t for n, t in with_flag.items() if "bubblechain" in n and n.endswith(".gfa")} == files
    assert sorted(with_flag) == sorted(list(without) + list(files) + [n[:-3] + "graphml" for n in files])
    assert all(with_flag[n] == t for n, t in without.items() if n.endswith(".gfa"))
    for i, chains in enumerate(per):                                     # the node attribute: j on the chain's nodes
        marked = {}
        for j, c in enumerate(chains):
            marked.update({graph.node_name(n): j for n in bu.nodes_of(want, order, c)})
        buf = __import__("io").StringIO()
        nodes = g.components.nodes_of(i).tolist()
        layout.write_graphml(buf, layout._ComponentView(graph, nodes, graph.edges[g.components.edges_of(i)]), marked)
        assert with_flag["component%d.graphml" % i] == buf.getvalue()
        assert with_flag["component%d.graphml" % i].count('<data key="d3">') == len(marked)
    # --min-nodes drops the short chains
    n_min = int(max(want["c_nodes"].tolist() + [1]))
    out = tmp_path / "out_min"
    assert cli.main(["chain-components", str(p), "-o", str(out), "--bubblechains", "--min-nodes", str(n_min)]) == 0
    assert sum(1 for f in out.iterdir() if "bubblechain" in f.name) == int((want["c_nodes"] >= n_min).sum())


def test_an_empty_graph_and_null_outputs():
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains(g)
    assert len(node_chain) == len(node_bubble) == len(edge_chain) == len(table) == 0 and ov.bubblechain_stats()["n_chains"] == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 4, 1, 1], [6, 6, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    lib = _lib.load()
    assert lib.po_layout_bubblechains(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 1
    st = ov.bubblechain_stats()
    assert (st["n_bubbles"], st["n_top"], st["n_chains"], st["n_short"], st["n_chain_nodes"], st["n_chain_edges"], st["max_chain_bubbles"]) == \
        (2, 2, 1, 0, 3, 2, 2)
    pos = np.full(4, 7, np.uint32)
    assert lib.po_layout_bubblechains(ov._h, g._ptr, None, None, pos.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(n)) == _lib.PO_OK
    assert pos.tolist() == [0, 1, 1, _lib.NO_NODE]
    edge = np.full(3, 7, np.uint32)
    prm = _lib.PoBubblechainParams(4, 0)
    assert lib.po_layout_bubblechains(ov._h, g._ptr, ctypes.byref(prm), None, None, edge.ctypes.data_as(ctypes.c_void_p), None,
                                      ctypes.byref(n)) == _lib.PO_OK
    assert n.value == 0 and edge.tolist() == [_lib.NO_NODE] * 3 and ov.bubblechain_stats()["n_short"] == 1
    g.free()
    ov.close()
