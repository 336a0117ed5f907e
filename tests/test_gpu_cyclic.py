"""The superbubbles of the whole graph, the cyclic partitions included, on the device (po_layout_superbubbles_all,
``layout.superbubbles(..., cyclic=True)``, ``chain-components --superbubbles --cyclic``) against
tests/golden/superbubble_all_cases.npz: the definition by brute force on the whole graph, held equal to the same per
partition and to the scheme by tests/make_cyclic_golden.py.  Exact integers throughout.  The one direct case with
merged-node ids cannot go through po_graph_from_edges; merged ids reach the device in every stage-(c) application here."""
import logging

import numpy as np
import pytest

import components_utils as cu
import cyclic_utils as cy
import superbubble_utils as su
from phasm_amd import _lib, layout
from test_cyclic_oracle import CASES, check_input, stage_inputs
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs
from test_gpu_components import FILE_CASES, segments
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text

pytestmark = pytest.mark.gpu

TEXT = [c for c in CASES if not c.get("direct")]
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1
UNIONS = ("direct_cy_four_node_digraphs_4096", "direct_cy_strong_union_2000")


def old_result(ov, res):
    """po_layout_superbubbles on the same result, in the shape of superbubble_utils.definition."""
    node_exit, node_inside, flags, table = ov.layout_superbubbles(res)
    none = lambda a: np.where(a == _lib.NO_NODE, su.NONE, a.astype(np.int64))   # noqa: E731
    return {"node_exit": none(node_exit), "node_inside": none(node_inside), "node_flags": flags.astype(np.int64),
            "b_entrance": table["entrance"].astype(np.int64), "b_exit": table["exit"].astype(np.int64),
            "b_inside": table["n_inside"].astype(np.int64), "b_nested": table["nested"].astype(np.int64)}


def check_all(ov, res, rec, want_inputs=None):
    """One application on the graph result ``res`` against its record; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    sb = layout.superbubbles(ov, res, cyclic=True)
    st = sb.stats
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    got = cy.as_result(st, (sb.node_exit, sb.node_inside, sb.node_flags, sb.table))
    cy.check_against_record(got, rec)                                                    # the golden: every array, every count
    want = cy.scheme_all(e[:, :2].tolist(), order.tolist())                              # the restatement, on the device's own edge order
    for k in cy.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: st[k] for k in cy.STAT_KEYS + cy.SCHEME_KEYS} == {k: want["stats"][k] for k in cy.STAT_KEYS + cy.SCHEME_KEYS}
    cy.check_singleton_part(got, old_result(ov, res), e[:, :2].tolist(), order.tolist())  # on singleton nodes: po_layout_superbubbles
    assert len(sb) == st["n_bubbles"] and st["n_invalid"] == 0 and st["n_nodes"] == len(order) and st["n_edges"] == len(e)
    assert st["n_certified"] <= st["n_rootless"] and (st["n_root_runs"] >= 1) == (len(order) > 0) and st["n_split_levels"] <= len(order) + 2
    if len(order):
        assert st["n_batches"] >= st["n_root_runs"] and st["n_scc_rounds"] >= st["n_split_levels"] + 1
    if want_inputs is not None:
        w_edges, w_order, _ = want_inputs
        assert order.tolist() == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: %d bubbles (%d cyclic), split %d in %d levels, %d rootless, %d runs, %d certified, %d filtered, %d SCC rounds, %d batches, "
          "%.3f ms (ranks %.3f, split %.3f, bubbles %.3f, merge %.3f)" % (
              rec["stage"], st["n_bubbles"], st["n_cyclic_bubbles"], st["n_split"], st["n_split_levels"], st["n_rootless"], st["n_root_runs"],
              st["n_certified"], st["n_edge_filtered"], st["n_scc_rounds"], st["n_batches"], st["ms_total"], st["ms_ranks"], st["ms_split"],
              st["ms_bubbles"], st["ms_merge"]))
    return sb.node_exit.tobytes() + sb.node_inside.tobytes() + sb.node_flags.tobytes() + sb.table.tobytes()


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_from_gfa_text_equals_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_b, rec_c = case["results"]
    final = cleaned(ov, edges_res)
    check_all(ov, final, rec_b, stages["b"])                               # (b) after the cleaning chain
    merged = ov.layout_merge(final)
    check_all(ov, merged, rec_c, stages["c"])                              # (c) the merged graph: node ids >= the reads
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
    check_input(inputs[0], inputs[1], case["results"][0])
    check_all(ov, g, case["results"][0], inputs)
    g.free()
    ov.close()


def test_the_two_unions_are_among_the_direct_cases():
    by = {c["name"]: c["results"][0] for c in DIRECT}
    assert by[UNIONS[0]]["n_nodes"] == 16384 and by[UNIONS[0]]["n_split"] > 4096          # past the prefix sum's first block
    assert by[UNIONS[1]]["n_rootless"] == 2000 and by[UNIONS[1]]["n_root_runs"] >= 3


def test_two_calls_and_a_fresh_handle_give_identical_bytes(tmp_path):
    case = next(c for c in TEXT if c["name"] == "selfish_1")
    seen = []
    for calls in (2, 1):
        ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
        final = cleaned(ov, edges_res)
        merged = ov.layout_merge(final)
        for _ in range(calls):
            seen.append(check_all(ov, final, case["results"][0]) + check_all(ov, merged, case["results"][1]))
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 3 and all(s == seen[0] for s in seen)
    for name in ("direct_cy_seven_nodes_lowest_0", "direct_cy_ring_of_16_diamonds_interior_lowest", "direct_k8_both_directions",
                 "direct_random_200_500_seed2", "direct_ring_1025_scrambled"):
        rnd = next(c for c in DIRECT if c["name"] == name)
        seen = []
        for calls in (2, 1):
            ov, g, _ = direct_graph(rnd)
            seen += [check_all(ov, g, rnd["results"][0]) for _ in range(calls)]
            g.free()
            ov.close()
        assert all(s == seen[0] for s in seen)


def test_the_call_takes_turns_with_its_siblings_on_one_handle():
    """The call works in the workspaces of po_layout_partition and po_layout_superbubbles, grown to twice the ranks: behind
    it, and behind a larger graph, both siblings and the call itself still give the bytes of a fresh handle."""
    names = ("direct_cy_seven_nodes_lowest_0", "direct_ring_1025_scrambled", "direct_sb_random_digraph_200_seed1")
    inputs = [stage_inputs(next(c for c in DIRECT if c["name"] == n))["a"] for n in names]
    n_ids = max(i[2] for i in inputs)

    def graph(ov, uv, order):
        return ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 1), 100), np.full((len(uv), 1), 17)], axis=1).astype(np.int64), order)

    calls = (lambda ov, g: ov.layout_partition(g), lambda ov, g: ov.layout_superbubbles(g), lambda ov, g: ov.layout_superbubbles_all(g))

    def fresh(call, uv, order):
        ov = segments(n_ids)
        g = graph(ov, uv, order)
        out = b"".join(a.tobytes() for a in call(ov, g))
        g.free()
        ov.close()
        return out

    ov = segments(n_ids)
    for uv, order, _ in inputs:
        g = graph(ov, uv, order)
        alone = [fresh(call, uv, order) for call in calls]
        for k in (0, 1, 2, 2, 1, 0):
            assert b"".join(a.tobytes() for a in calls[k](ov, g)) == alone[k], k
        g.free()
    ov.close()


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_command_logs_the_superbubbles_of_all_partitions(name, tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in TEXT if c["name"] == name)
    rec = case["results"][1]
    text = component_stage_inputs(next(c for c in COMPONENT_CASES if c["name"] == name))["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    g = layout.chain_components(str(p), superbubbles=True, cyclic=True)
    plain = layout.chain_components(str(p), superbubbles=True)
    assert plain.superbubbles_all is None and plain.superbubbles.table.tobytes() == g.superbubbles.table.tobytes()
    # the file numbers its nodes by its own S lines: the stage-(c) graph under other ids than the golden's.  The arrays are
    # the restatement's on the file's own graph; the counts are the golden's, whatever the numbering
    graph = g.graph
    want = cy.scheme_all(graph.edges[:, :2].tolist(), graph.node_order)
    sb = g.superbubbles_all
    got = cy.as_result(sb.stats, (sb.node_exit, sb.node_inside, sb.node_flags, sb.table))
    for k in cy.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: sb.stats[k] for k in cy.STAT_KEYS} == {k: rec[k] for k in cy.STAT_KEYS}
    weak = cu.weak_components(graph.edges, graph.node_order)
    comp_of = dict(zip([int(x) for x in graph.node_order], weak["node_component"].tolist()))
    n = weak["stats"]["n_components"]
    per, cyc = [0] * n, [0] * n
    acyclic = set(g.superbubbles.table["entrance"].tolist())
    for s in want["b_entrance"].tolist():
        per[comp_of[s]] += 1
        cyc[comp_of[s]] += s not in acyclic
    assert sum(cyc) == rec["n_cyclic_bubbles"]
    lines_want = ["Connected component %d: %d superbubbles in all its partitions, %d of them in non-singleton SCCs." % (i, per[i], cyc[i])
                  for i in range(n)]
    outs = {}
    mine = lambda m: m.startswith("Connected component") and "all its partitions" in m   # noqa: E731
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["chain-components", str(p), "-o", str(out), "-f", "gfa2", "--superbubbles"] + (["--cyclic"] if flag else [])) == 0
        lines = [r.getMessage() for r in caplog.records if mine(r.getMessage())]
        assert lines == (lines_want if flag else [])
        outs[flag] = ({f.name: f.read_bytes() for f in sorted(out.iterdir())}, [r.getMessage() for r in caplog.records if not mine(r.getMessage())])
    assert outs[True] == outs[False]                                        # with the flag: today's lines and files, plus the new lines


def test_an_empty_graph_and_null_outputs():
    import ctypes
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    node_exit, node_inside, flags, table = ov.layout_superbubbles_all(g)
    assert len(node_exit) == len(node_inside) == len(flags) == len(table) == 0 and ov.superbubble_all_stats()["n_bubbles"] == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 4, 1, 1], [4, 0, 1, 1], [6, 6, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    lib = _lib.load()
    assert lib.po_layout_superbubbles_all(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 3
    st = ov.superbubble_all_stats()
    assert (st["n_bubbles"], st["n_cyclic_bubbles"], st["n_rootless"], st["n_root_runs"], st["n_certified"], st["n_split"]) == (3, 3, 1, 1, 1, 1)
    flags = np.zeros(4, np.uint8)
    assert lib.po_layout_superbubbles_all(ov._h, g._ptr, None, None, None, flags.ctypes.data_as(ctypes.c_void_p), None,
                                          ctypes.byref(n)) == _lib.PO_OK
    assert flags.tolist() == [_lib.SB_ENTRANCE | _lib.SB_EXIT] * 3 + [_lib.SB_SELF_LOOP]
    g.free()
    ov.close()
