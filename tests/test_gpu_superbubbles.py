"""The superbubbles of the acyclic partitions on the device (po_layout_superbubbles, layout.superbubbles,
``chain-components --superbubbles``) against tests/golden/superbubble_cases.npz: the reference's partition_graph,
SuperBubbleFinderDAG and superbubble_nodes, unmodified, on the reference's graphs at two stages and on the direct cases.
Exact integers throughout.  The one direct case with merged-node ids cannot go through po_graph_from_edges (its ends are
oriented reads by contract); merged ids reach the device in every stage-(c) application here, and
tests/test_superbubbles_host_emulation.py runs the kernels on the case itself."""
import logging

import numpy as np
import pytest

import components_utils as cu
import partition_utils as pu
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs
from test_gpu_components import FILE_CASES, merge_bytes, segments
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text
from test_superbubbles_oracle import CASES, check_reference, stage_inputs

pytestmark = pytest.mark.gpu

TEXT = [c for c in CASES if not c.get("direct")]
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1


def as_result(sb):
    node = lambda a: np.where(a == _lib.NO_NODE, su.NONE, a.astype(np.int64))   # noqa: E731
    t = sb.table
    return {"node_exit": node(sb.node_exit), "node_inside": node(sb.node_inside), "node_flags": sb.node_flags.astype(np.int64),
            "b_entrance": t["entrance"].astype(np.int64), "b_exit": t["exit"].astype(np.int64), "b_inside": t["n_inside"].astype(np.int64),
            "b_nested": t["nested"].astype(np.int64), "stats": dict(sb.stats)}


def check_superbubbles(ov, res, rec, want_inputs=None):
    """One application on the graph result ``res`` against its record; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    sb = layout.superbubbles(ov, res)
    st = sb.stats
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    got = as_result(sb)
    su.check_against_record(got, rec)                                                    # the golden: the contract's arrays
    sets = [sorted(sb.nodes(s).tolist()) for s, _ in sb.pairs()]
    check_reference(got, sets, e, order.tolist(), rec)                                   # ... and the reference's pairs and node sets
    want = su.scheme(e, order.tolist())                                                  # the restatement, on the device's own edge order
    for k in su.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert sets == su.node_sets(want, order.tolist()) and len(sb) == st["n_bubbles"]
    assert sb.pairs(nested=False) == [p for p, nested in zip(sb.pairs(), want["b_nested"].tolist()) if not nested]
    # the stats are consistent: rounds stay within the caps, batches within what the loops allow (no particular count is asserted)
    n = len(order)
    n_real = st["n_p_nodes"]
    assert st["n_invalid"] == 0 and st["n_nodes"] == n and st["n_edges"] == len(e)
    assert (st["n_levels_forward"], st["n_levels_backward"]) == (rec["n_levels_forward"], rec["n_levels_backward"])
    assert st["n_levels_forward"] <= n_real <= n + 2
    if n:
        assert 1 <= st["n_level_rounds"] <= max(st["n_levels_forward"], st["n_levels_backward"], 1) + 1 <= n_real + 2
        assert st["n_discard_rounds"] <= rec["n_discard_rounds"] + 0 and st["n_discard_rounds"] <= n_real + 2
        assert (st["n_discard_rounds"] > 0) == (st["n_self_loop_nodes"] > 0)
        part = pu.partition_rounds(e, order.tolist())["stats"]
        assert st["n_scc_rounds"] <= part["n_outer"] * 3 * (n + 2)
        rounds = st["n_scc_rounds"] + st["n_level_rounds"] + st["n_discard_rounds"]
        assert -(-rounds // 8) <= st["n_batches"] <= rounds // 8 + 3 * part["n_outer"] + 2      # (at most one part-filled batch per loop)
    if want_inputs is not None:
        w_edges, w_order, _ = want_inputs
        assert order.tolist() == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: %d bubbles, levels %d / %d, rounds %d + %d + %d, %d batches, %.3f ms (partition %.3f, levels %.3f, dominators %.3f, label %.3f)" % (
        rec["stage"], st["n_bubbles"], st["n_levels_forward"], st["n_levels_backward"], st["n_scc_rounds"], st["n_level_rounds"],
        st["n_discard_rounds"], st["n_batches"], st["ms_total"], st["ms_partition"], st["ms_levels"], st["ms_dominators"], st["ms_label"]))
    return sb.node_exit.tobytes() + sb.node_inside.tobytes() + sb.node_flags.tobytes() + sb.table.tobytes()


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_superbubbles_from_gfa_text_equal_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_b, rec_c = case["results"]
    final = cleaned(ov, edges_res)
    merge_before = merge_bytes(ov, final)
    check_superbubbles(ov, final, rec_b, stages["b"])                      # (b) after the cleaning chain
    assert merge_bytes(ov, final) == merge_before                          # a merge after the call gives the same bytes
    merged = ov.layout_merge(final)
    check_superbubbles(ov, merged, rec_c, stages["c"])                     # (c) the merged graph: node ids >= the reads
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
    check_superbubbles(ov, g, case["results"][0], inputs)
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
            seen.append(check_superbubbles(ov, final, case["results"][0]) + check_superbubbles(ov, merged, case["results"][1]))
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 4 and all(s == seen[0] for s in seen)
    for name in ("direct_sb_random_dag_200_seed0", "direct_sb_random_digraph_200_seed1", "direct_sb_fan_out_and_in_257"):
        rnd = next(c for c in DIRECT if c["name"] == name)
        seen = []
        for calls in (3, 1):
            ov, g, _ = direct_graph(rnd)
            seen += [check_superbubbles(ov, g, rnd["results"][0]) for _ in range(calls)]
            g.free()
            ov.close()
        assert all(s == seen[0] for s in seen)


TURN_NAMES = ("direct_three_cycle_with_tails", "direct_sb_path_1025_scrambled", "direct_sb_random_digraph_200_seed1")   # small, large, small


def test_components_partition_and_superbubbles_take_turns_on_one_handle():
    """The three calls rank the graph in the same buffers of the handle, and the superbubbles run the SCC stage in the
    workspaces of the partition: on one handle they alternate, twice each, on a few nodes, then 1 025, then 200, so every
    call finds what a call of another stage -- and, behind the large graph, of a larger graph -- left there.  Every call's
    arrays are the restatements', and its bytes those of the same call on a handle that has run nothing else."""
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

    def superbubbles(ov, g):
        node_exit, node_inside, flags, table = ov.layout_superbubbles(g)
        none = lambda a: np.where(a == _lib.NO_NODE, su.NONE, a.astype(np.int64))   # noqa: E731
        return {"node_exit": none(node_exit), "node_inside": none(node_inside), "node_flags": flags, "b_entrance": table["entrance"],
                "b_exit": table["exit"], "b_inside": table["n_inside"], "b_nested": table["nested"]}

    def fresh(call, uv, order):
        ov = segments(n_ids)
        g = graph(ov, uv, order)
        out = call(ov, g)
        g.free()
        ov.close()
        return out

    calls = (components, partition, superbubbles)
    ov = segments(n_ids)
    for uv, order, _ in inputs:
        g = graph(ov, uv, order)
        e = edge_array(g.rows())
        want = {components: cu.weak_components(e[:, :2], list(order)), partition: pu.partition(e, list(order)),
                superbubbles: su.scheme(e, list(order))}
        alone = {call: fresh(call, uv, order) for call in calls}
        for call in calls + calls[::-1]:
            got = call(ov, g)
            assert set(got) == set(alone[call]) and len(got) >= 5
            for k, a in got.items():
                assert a.tolist() == np.asarray(want[call][k]).tolist(), (call.__name__, k)
                assert a.dtype == alone[call][k].dtype and a.tobytes() == alone[call][k].tobytes(), (call.__name__, k)
        g.free()
    ov.close()


def expected_lines(sb_want, weak, order):
    comp_of = dict(zip([int(x) for x in order], weak["node_component"].tolist()))
    n = weak["stats"]["n_components"]
    per, top = [0] * n, [0] * n
    for s, nested in zip(sb_want["b_entrance"].tolist(), sb_want["b_nested"].tolist()):
        per[comp_of[s]] += 1
        top[comp_of[s]] += not nested
    return ["Connected component %d: %d superbubbles in its acyclic partition, %d of them not nested." % (i, per[i], top[i]) for i in range(n)]


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_file_route_equals_the_reference(name, tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in TEXT if c["name"] == name)
    rec = case["results"][1]
    text = component_stage_inputs(next(c for c in COMPONENT_CASES if c["name"] == name))["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    g = layout.chain_components(str(p), superbubbles=True)
    plain = layout.chain_components(str(p))
    assert plain.superbubbles is None and plain.partitions is None and g.partitions is None
    assert plain.components.component_of_node.tobytes() == g.components.component_of_node.tobytes()
    # the file numbers its nodes by its own S lines: the stage-(c) graph under other ids than the golden's.  The arrays are
    # the restatement's on the file's own graph; the counts are the golden's, whatever the numbering
    graph = g.graph
    assert len(graph.node_order) == rec["n_nodes"] and len(graph.edges) == rec["n_edges"]
    want = su.scheme(graph.edges, graph.node_order)
    got = as_result(g.superbubbles)
    for k in su.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: g.superbubbles.stats[k] for k in su.STAT_KEYS} == {k: rec[k] for k in su.STAT_KEYS}
    if "a_b_inside" in rec:
        assert sorted(got["b_inside"].tolist()) == sorted(rec["a_b_inside"]) and sorted(got["b_nested"].tolist()) == sorted(rec["a_b_nested"])
    # the command: with the flag one line per component; without it today's output and files
    weak = cu.weak_components(graph.edges, graph.node_order)
    outs = {}
    mine = lambda m: m.startswith("Connected component") and "superbubbles" in m   # noqa: E731
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["chain-components", str(p), "-o", str(out), "-f", "gfa2,graphml"] + (["--superbubbles"] if flag else [])) == 0
        lines = [r.getMessage() for r in caplog.records if mine(r.getMessage())]
        assert lines == (expected_lines(want, weak, graph.node_order) if flag else [])
        outs[flag] = ({f.name: f.read_bytes() for f in sorted(out.iterdir())}, [r.getMessage() for r in caplog.records if not mine(r.getMessage())])
    assert outs[True] == outs[False] and len(outs[False][0]) == 2 * len(g.components)


def test_an_empty_graph_and_null_outputs():
    import ctypes
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    node_exit, node_inside, flags, table = ov.layout_superbubbles(g)
    assert len(node_exit) == len(node_inside) == len(flags) == len(table) == 0 and ov.superbubble_stats()["n_bubbles"] == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 4, 1, 1], [6, 6, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    lib = _lib.load()
    assert lib.po_layout_superbubbles(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 2
    st = ov.superbubble_stats()
    assert (st["n_bubbles"], st["n_nested"], st["n_self_loop_nodes"], st["n_p_nodes"], st["n_p_edges"]) == (2, 0, 1, 6, 5)
    flags = np.zeros(4, np.uint8)
    assert lib.po_layout_superbubbles(ov._h, g._ptr, None, None, None, flags.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(n)) == _lib.PO_OK
    assert flags.tolist() == [_lib.SB_ENTRANCE, _lib.SB_ENTRANCE | _lib.SB_EXIT, _lib.SB_EXIT, _lib.SB_SELF_LOOP]
    g.free()
    ov.close()
