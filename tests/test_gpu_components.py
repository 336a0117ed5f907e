"""Weakly connected components on the device (po_layout_components, po_graph_from_edges, layout.weakly_connected_components,
layout.chain_components, ``chain-components``) against tests/golden/components_cases.npz: networkx on the reference's
graphs at three stages, the reference's reconstruction of the graph files it wrote, and its writers.  Exact integers
throughout.  The one direct case with merged-node ids cannot go through po_graph_from_edges (its ends are oriented reads
by contract); merged ids reach the device in every stage-(c) application here, and tests/test_components_host_emulation.py
runs the kernels on the case itself."""
import logging

import numpy as np
import pytest

import components_utils as cu
from phasm_amd import layout
from phasm_amd.overlapper import ExactOverlapper
from test_components_oracle import CASES, GOLDEN, file_route, stage_inputs
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text

pytestmark = pytest.mark.gpu

TEXT = [c for c in CASES if not c.get("direct")]
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1


def as_result(nodes, edges, table, st):
    return {"node_component": nodes.tolist(), "edge_component": edges.tolist(), "first_node": table["first_node"].tolist(),
            "n_nodes": table["n_nodes"].tolist(), "n_edges": table["n_edges"].tolist(), "stats": st}


def check_components(ov, res, rec, want_inputs=None):
    """One application on the graph result ``res`` against its record; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    nodes, edges, table = ov.layout_components(res)
    st = ov.components_stats()
    got = as_result(nodes, edges, table, st)
    cu.check_against_record(got, rec)
    assert st["n_invalid"] == 0 and st["n_rounds"] <= len(order) + 2 and (st["n_rounds"] > 0) == (len(order) > 0)
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    want = cu.weak_components(e, order.tolist())
    assert got["edge_component"] == want["edge_component"].tolist() and got["node_component"] == want["node_component"].tolist()
    if want_inputs is not None:
        w_edges, w_order, _ = want_inputs
        assert order.tolist() == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: n_rounds %d (synchronous %d), %d batches, %.3f ms" % (rec["stage"], st["n_rounds"], rec["rounds"], st["n_batches"], st["ms_total"]))
    return nodes.tobytes() + edges.tobytes() + table.tobytes()


def merge_bytes(ov, res):
    merged, flags = ov.layout_merge(res, want_flags=True)
    out = [flags.tobytes(), merged.rows().tobytes(), merged.node_order().tobytes()] + [t.tobytes() for t in merged.merged_paths()]
    merged.free()
    return out


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_components_from_gfa_text_equal_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_a, rec_b, rec_c = case["results"]
    check_components(ov, edges_res, rec_a, stages["a"])                    # (a) the stage-1 graph
    final = cleaned(ov, edges_res)
    merge_before = merge_bytes(ov, final)
    check_components(ov, final, rec_b, stages["b"])                        # (b) after the cleaning chain
    assert merge_bytes(ov, final) == merge_before                          # a merge after the call gives the same bytes
    merged = ov.layout_merge(final)
    check_components(ov, merged, rec_c, stages["c"])                       # (c) the merged graph: node ids >= the reads
    assert len(ov) == rec_c["n_ids"]
    for r in (merged, final, edges_res):
        r.free()
    ov.close()


def segments(n_ids):
    ov = ExactOverlapper()
    for i in range(n_ids // 2):
        ov.add_segment("s%d" % i, 1000 + i % 97)
    return ov


@pytest.mark.parametrize("case", DIRECT, ids=[c["name"] for c in DIRECT])
def test_direct_cases_through_graph_from_edges(case):
    rec = case["results"][0]
    uv, order, n_ids = stage_inputs(case)["a"]
    ov = segments(n_ids)
    e = np.concatenate([uv, np.full((len(uv), 1), 100), np.full((len(uv), 1), 17)], axis=1).astype(np.int64)
    g = ov.graph_from_edges(e, order)
    assert len(g) == len(uv) and g.node_order().tolist() == list(order)
    assert edge_array(g.rows()).tolist() == e.tolist() if len(e) else len(g.rows()) == 0
    check_components(ov, g, rec, (uv, order, n_ids))
    comps = layout.weakly_connected_components(ov, g)
    assert len(comps) == rec["n_components"] and comps.node_order.tolist() == list(order)
    want = cu.weak_components(uv, order)
    for i in range(min(len(comps), 5)):
        assert comps.edges_of(i).tolist() == np.flatnonzero(want["edge_component"] == i).tolist()
        assert comps.nodes_of(i).tolist() == [n for n, c in zip(order, want["node_component"].tolist()) if c == i]
    g.free()
    ov.close()


def test_three_calls_and_a_fresh_handle_give_identical_bytes(tmp_path):
    case = next(c for c in TEXT if c["name"] == "union_21_1")
    seen = []
    for calls in (3, 1):
        ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
        final = cleaned(ov, edges_res)
        for _ in range(calls):
            seen.append(check_components(ov, edges_res, case["results"][0]) + check_components(ov, final, case["results"][1]))
        for r in (final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 4 and all(s == seen[0] for s in seen)
    path = next(c for c in DIRECT if c["name"] == "direct_path_4097_scrambled")
    uv, order, n_ids = stage_inputs(path)["a"]
    e = np.concatenate([uv, np.full((len(uv), 2), 1)], axis=1)
    seen = []
    for calls in (3, 1):
        ov = segments(n_ids)
        g = ov.graph_from_edges(e, order)
        seen += [check_components(ov, g, path["results"][0]) for _ in range(calls)]
        g.free()
        ov.close()
    assert all(s == seen[0] for s in seen)


FILE_CASES = ["union_21_1", "selfish_2", "reduced_line_101", "ring_40", "lasso_70_6", "tangle_3"]


def check_chain(text, rec, tmp_path, formats):
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    graph = file_route(text, rec)                                          # (the reader against the golden, as on the CPU)
    g = layout.chain_components(str(p))
    assert g.graph.node_order == rec["file_order"] and g.graph.edges.tolist() == graph.edges.tolist()
    comps = g.components
    got = as_result(comps.component_of_node, comps.component_of_edge, comps.table, comps.stats)
    cu.check_against_record(got, rec)
    out = tmp_path / "out"
    assert layout.write_component_graphs(str(out), g, formats) == rec["n_components"]
    return g, out


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_file_route_equals_the_reference(name, tmp_path):
    case = next(c for c in TEXT if c["name"] == name)
    rec = case["file"]
    g, out = check_chain(stage_inputs(case)["file"], rec, tmp_path, ("gfa2",))
    (tmp_path / "one").mkdir()
    _, out1 = check_chain(stage_inputs(case)["file"], rec, tmp_path / "one", ("gfa2", "gfa1", "graphml"))
    written = [((out / ("component%d.gfa" % i)).read_text().splitlines(True), (out1 / ("component%d.gfa" % i)).read_text().splitlines(True))
               for i in range(rec["n_components"])]
    assert cu.writers_digest(written) == rec["writers_sha256"]             # gfa2 alone; gfa1 after gfa2: the later one wins
    import networkx
    for i in range(rec["n_components"]):
        x = networkx.read_graphml(str(out1 / ("component%d.graphml" % i)))
        assert (x.number_of_nodes(), x.number_of_edges()) == (rec["c_n_nodes"][i], rec["c_n_edges"][i])


@pytest.mark.parametrize("rec", GOLDEN["hand_files"], ids=[r["name"] for r in GOLDEN["hand_files"]])
def test_the_file_route_on_the_hand_written_files(rec, tmp_path):
    check_chain(cu.HAND_FILES[rec["name"]], rec, tmp_path, ("gfa1",))


def test_the_command_writes_the_components_and_warns(tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in TEXT if c["name"] == "selfish_2")
    rec = case["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(stage_inputs(case)["file"])
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger=cli.logger.name):
        assert cli.main(["chain-components", str(p), "-o", str(out), "-f", "gfa2, svg ,graphml"]) == 0
    assert "File format 'svg' not recognised, ignoring." in caplog.text
    for i in range(rec["n_components"]):
        assert "Connected component %d with %d nodes and %d edges." % (i, rec["c_n_nodes"][i], rec["c_n_edges"][i]) in caplog.text
    assert sorted(f.name for f in out.iterdir()) == sorted("component%d.%s" % (i, ext) for i in range(rec["n_components"])
                                                            for ext in ("gfa", "graphml"))
    with pytest.raises(SystemExit) as exc:
        cli.main(["chain-components", str(p), "-o", str(tmp_path / "none"), "-f", "svg"])
    assert exc.value.code == 1 and not (tmp_path / "none").exists()
