"""Average coverage per edge on the device (po_layout_coverage; layout.average_coverage, ``coverage=True``, ``layout-edges
--coverage / --graphml``) against the golden applications that the reference's own average_coverage_path produced
(tests/golden/coverage_cases.npz).  Exact integers, and float64 quotients compared bit for bit."""
import ctypes
import logging
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import coverage_utils as cu
import golden_utils as gu
import tips_utils as tu
from phasm_amd import _lib, layout
from phasm_amd.overlapper import ExactOverlapper
from test_coverage_oracle import CASES
from test_gpu_merge import cleaned, edge_array

pytestmark = pytest.mark.gpu

BY_NAME = {c["name"]: c for c in CASES}


def open_case(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(cu.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    return ov, rows, edges_res


def check_coverage(ov, graph_res, rows_res, case, rec):
    """One application against its record; returns the bytes of the result."""
    before, rows_before = graph_res.rows().tobytes(), rows_res.rows().tobytes()
    e = edge_array(graph_res.rows())
    o = tu.by_uv(e)
    sums = ov.layout_coverage(graph_res, rows_res)
    st = ov.coverage_stats()
    avg = layout.average_coverage(ov, graph_res, rows_res)
    assert avg.dtype == np.float64
    cu.check_record(rec, e[o][:, 0], e[o][:, 1], sums["read_length_sum"][o], sums["path_length"][o], avg[o])
    if len(e):
        assert (st["n_edges"], st["n_rows"], st["n_nodes"], st["n_pairs"], st["max_set"], st["n_zero_path"], st["n_invalid"]) == \
               (len(e), len(rows_res), rec["n_nodes"], rec["n_pairs"], rec["max_set"], 0, 0)
    assert graph_res.rows().tobytes() == before and rows_res.rows().tobytes() == rows_before   # the inputs stay as they were
    return sums.tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_coverage_from_gfa_text_equals_the_reference(case, tmp_path):
    ov, rows, edges_res = open_case(case, tmp_path)
    rec_a, rec_b = case["results"]
    check_coverage(ov, edges_res, rows, case, rec_a)                          # (a) on the stage-1 graph
    final = cleaned(ov, edges_res)
    merged = ov.layout_merge(final)
    check_coverage(ov, merged, rows, case, rec_b)                             # (b) on the merged graph
    for r in (merged, final, edges_res, rows):
        r.free()
    ov.close()


ENTRY = ["union_21_1", "reduced_hub_1024", "selfish_2", "lasso_70_6", "stem_1", "giant_1", "mix_1"]


def graphml_graph(path):
    ns = "{http://graphml.graphdrawing.org/xmlns}"
    root = ET.parse(str(path)).getroot()
    keys = {k.get("id"): k.get("attr.name") for k in root.iter(ns + "key")}
    nodes = [n.get("id") for n in root.iter(ns + "node")]
    edges = {}
    for e in root.iter(ns + "edge"):
        d = {keys[x.get("key")]: x.text for x in e.iter(ns + "data")}
        edges[(e.get("source"), e.get("target"))] = (int(d["weight"]), int(d["overlap_len"]), float(d["avg_coverage"]))
        assert set(d) == {"weight", "overlap_len", "avg_coverage"}
    return nodes, edges


@pytest.mark.parametrize("name", ENTRY)
def test_the_entry_points_and_the_cli_give_the_same_bytes(name, tmp_path, caplog):
    from phasm_amd import cli
    case = BY_NAME[name]
    rec_a, rec_b = case["results"]
    ov, rows, edges_res = open_case(case, tmp_path)
    final = cleaned(ov, edges_res)
    merged = ov.layout_merge(final)
    direct = layout.average_coverage(ov, merged, rows)
    direct_sums = ov.layout_coverage(merged, rows)
    stage1 = layout.average_coverage(ov, edges_res, rows)
    chained = layout.clean_assembly_graph(ov, edges_res, merge=True, coverage=True, rows=rows)
    plain = layout.clean_assembly_graph(ov, edges_res, merge=True)
    with pytest.raises(ValueError):
        layout.clean_assembly_graph(ov, edges_res, merge=True, coverage=True)
    merged.free()
    final.free()
    edges_res.free()
    rows.free()
    ov.close()
    assert plain.coverage_sums is None and plain.avg_coverage is None and plain.coverage_stats is None
    assert chained.edges.tobytes() == plain.edges.tobytes()
    assert chained.avg_coverage.tobytes() == direct.tobytes() and chained.coverage_sums.tobytes() == direct_sums.tobytes()
    assert (chained.coverage_stats["n_pairs"], chained.coverage_stats["max_set"]) == (rec_b["n_pairs"], rec_b["max_set"]) or not len(direct)
    p = tmp_path / "in.gfa"
    params = dict(case["params"])
    from_file = layout.layout_from_gfa(str(p), merge=True, coverage=True, **params)
    assert from_file.avg_coverage.tobytes() == direct.tobytes() and from_file.edges.tobytes() == plain.edges.tobytes()
    first = layout.layout_from_gfa(str(p), coverage=True, **params)
    assert first.avg_coverage.tobytes() == stage1.tobytes() and first.merged_paths is None
    assert layout.layout_from_gfa(str(p), merge=True, **params).avg_coverage is None
    # the CLI: the reference's log line, the GFA2 file unchanged by the options, the GraphML beside it
    argv = ["-l", str(params["min_read_length"]), "-s", str(params["min_overlap_length"]), "-a", str(params["max_overhang_abs"]),
            "-r", repr(params["max_overhang_rel"])]
    for step, want_g in (("--merge", chained), (None, first)):
        tag = step or "stage1"
        out0, out1, out2, gml = (tmp_path / (tag + x) for x in (".gfa", ".cov.gfa", ".gml.gfa", ".graphml"))
        extra = [step] if step else []
        assert cli.main(["layout-edges", str(p), "-o", str(out0)] + extra + argv) == 0
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["layout-edges", str(p), "--coverage", "-o", str(out1)] + extra + argv) == 0
        assert "Calculating average coverage for each edge..." in [r.getMessage() for r in caplog.records]
        assert cli.main(["layout-edges", str(p), "--graphml", str(gml), "-o", str(out2)] + extra + argv) == 0
        assert out0.read_bytes() == out1.read_bytes() == out2.read_bytes()
        nodes, edges = graphml_graph(gml)
        want = {(u, v): (w, o, c) for (u, v, w, o), c in zip(want_g.edge_tuples(), want_g.avg_coverage.tolist())}
        assert edges == want and len(set(nodes)) == len(nodes)
        ends = {n for uv in want for n in uv}
        if want_g.node_order is not None:
            assert nodes == [want_g.node_name(n) for n in want_g.node_order.tolist()] and ends <= set(nodes)
        else:
            assert set(nodes) == ends
        try:
            import networkx
        except ImportError:
            continue
        g, mine = networkx.read_graphml(str(gml)), want_g.to_networkx()
        assert {(u, v): (d["weight"], d["overlap_len"], d["avg_coverage"]) for u, v, d in g.edges(data=True)} == \
               {(u, v): (d["weight"], d["overlap_len"], d["avg_coverage"]) for u, v, d in mine.edges(data=True)} == want


def test_the_cli_reads_dump_text_too(tmp_path):
    """--coverage and --graphml from --las: DBdump + LAdump text gives the file that the same alignments give as GFA2 text,
    and what ``layout_from_daligner(coverage=True)`` and the plain statement compute."""
    import io
    import json
    import os
    from phasm_amd import cli
    from phasm_amd.io import gfa
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "daligner_cases.json")))
    done = 0
    for case in d["cases"]:
        if "ok" not in case["gfa"] or case["name"] in ("no_reads", "trace_empty_list") or case["translations"]:
            continue
        params = dict(layout.DEFAULTS, max_overhang_abs=20, max_overhang_rel=0.3)
        direct = layout.layout_from_daligner(io.StringIO(case["db"]), io.StringIO(case["las"]), None, coverage=True, **params)
        if not len(direct.edges):
            continue
        _, lengths, rows = gfa.read_gfa2_rows(io.StringIO(case["gfa"]["ok"]))
        want = cu.edge_coverage(rows, edge_array(direct.edges), {}, np.repeat(lengths, 2).tolist())
        assert direct.coverage_sums["read_length_sum"].tolist() == want[0].tolist()
        assert direct.avg_coverage.tobytes() == want[2].tobytes()
        sub = tmp_path / case["name"]
        sub.mkdir()
        (sub / "db.txt").write_text(case["db"])
        (sub / "las.txt").write_text(case["las"])
        (sub / "in.gfa").write_text(case["gfa"]["ok"])
        common = ["layout-edges", "-a", "20", "-r", "0.3"]
        assert cli.main(common + [str(sub / "db.txt"), "--las", str(sub / "las.txt"), "--graphml", str(sub / "1.graphml"),
                                  "-o", str(sub / "1.gfa")]) == 0
        assert cli.main(common + [str(sub / "in.gfa"), "--coverage", "--graphml", str(sub / "2.graphml"), "-o", str(sub / "2.gfa")]) == 0
        assert (sub / "1.graphml").read_bytes() == (sub / "2.graphml").read_bytes()
        nodes, edges = graphml_graph(sub / "1.graphml")
        assert edges == {(u, v): (w, o, c) for (u, v, w, o), c in zip(direct.edge_tuples(), direct.avg_coverage.tolist())}
        done += 1
    assert done > 0


def test_a_zero_path_length_raises_like_the_reference():
    sums = np.zeros(2, dtype=_lib.COVERAGE_DTYPE)
    sums["read_length_sum"], sums["path_length"] = [6, 5], [4, 0]
    with pytest.raises(ZeroDivisionError):
        layout._quotients(sums)
    sums["path_length"][1] = -2
    assert layout._quotients(sums).tolist() == [1.5, -2.5]


LADDERS = [c for c in CASES if c.get("reduce_case") in ("ladder_varlen", "ladder_cfg2_mini")]


@pytest.mark.parametrize("case", LADDERS, ids=[c["name"] for c in LADDERS])
def test_ladder_straight_from_overlap_rows_with_and_without_the_table(case, monkeypatch):
    """The rows of po_overlaps never leave HBM; the expectation is the plain statement on the rows read back."""
    _, seqs, m, _ = gu.ladder_case(case["reduce_case"])
    ov = ExactOverlapper()
    for i in range(len(seqs) // 2):
        ov.add_sequence("read%d+" % i, seqs[2 * i])
        ov.add_sequence("read%d-" % i, seqs[2 * i + 1])
    res = ov.overlaps_result(m)
    r = res.rows()
    rows = np.stack([r[f] for f in r.dtype.names], 1).astype(np.int64)
    L = ov.lengths().tolist()
    seen = []
    for table in (False, True):
        if table:
            monkeypatch.setenv("PHASM_LAYOUT_TABLE", "1")
        else:
            monkeypatch.delenv("PHASM_LAYOUT_TABLE", raising=False)
        edges_res, _ = ov.layout_edges(res, **case["params"])
        final = cleaned(ov, edges_res)
        merged = ov.layout_merge(final)
        offsets, members, _, mlen = merged.merged_paths()
        mem = {len(L) + k: members[offsets[k]:offsets[k + 1]].tolist() for k in range(len(mlen))}
        for graph_res, mm, ll in ((edges_res, {}, L), (merged, mem, L + mlen.tolist())):
            e = edge_array(graph_res.rows())
            sums = ov.layout_coverage(graph_res, res)
            st = ov.coverage_stats()
            want = cu.edge_coverage(rows, e, mm, ll)
            assert sums["read_length_sum"].tolist() == want[0].tolist() and sums["path_length"].tolist() == want[1].tolist()
            assert layout.average_coverage(ov, graph_res, res).tobytes() == want[2].tobytes()
            assert (st["n_nodes"], st["n_pairs"], st["max_set"]) == cu.set_stats(rows, e, mm)
            o = tu.by_uv(e)
            seen.append((e[o].tobytes(), sums[o].tobytes()))
        for x in (merged, final, edges_res):
            x.free()
    assert seen[:2] == seen[2:] and len(seen[0][1]) > 0
    assert res.rows().tobytes() == r.tobytes()
    res.free()
    ov.close()


def test_interleaved_calls_on_one_handle_and_the_error_cases(tmp_path):
    """The workspaces of the coverage live on the handle beside those of the merge, the tips and the diamonds."""
    held = []
    for name in ("reduced_hub_1025", "stem_1"):
        d = tmp_path / name
        d.mkdir()
        held.append(open_case(BY_NAME[name], d))
    for ov, rows, edges_res in held:
        seen = set()
        for _ in range(5):
            c1 = ov.layout_coverage(edges_res, rows)
            reduced = ov.layout_reduce(edges_res, 1000)
            tipped = ov.layout_tips(reduced)
            c2 = ov.layout_coverage(tipped, rows)
            kept = ov.layout_diamonds(tipped)
            merged = ov.layout_merge(kept)
            c3 = ov.layout_coverage(merged, rows)
            c4 = ov.layout_coverage(edges_res, rows)
            assert c1.tobytes() == c4.tobytes()
            seen.add((c1.tobytes(), c2.tobytes(), c3.tobytes()))
            for r in (merged, kept, tipped, reduced):
                r.free()
        assert len(seen) == 1 and all(len(x) for x in next(iter(seen))[:2])
    ov, rows, edges_res = held[0]
    other = ExactOverlapper()
    other.add_segment("x", 10)
    other_rows = other.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    for graph, rr in ((rows, rows), (edges_res, edges_res), (edges_res, other_rows)):
        with pytest.raises(ValueError):                                       # the wrong kind in either position, another handle
            ov.layout_coverage(graph, rr)
    with pytest.raises(ValueError):
        other.layout_coverage(edges_res, other_rows)
    lib = _lib.load()
    out = np.zeros(len(edges_res), dtype=_lib.COVERAGE_DTYPE)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.po_layout_coverage(ov._h, edges_res._ptr, rows._ptr, ctypes.byref(_lib.PoCoverageParams(1)), ptr) == _lib.PO_ERR_INVALID
    assert lib.po_layout_coverage(ov._h, edges_res._ptr, rows._ptr, None, None) == _lib.PO_ERR_INVALID
    assert not out["path_length"].any()
    assert lib.po_layout_coverage(ov._h, edges_res._ptr, rows._ptr, None, ptr) == _lib.PO_OK      # params may be NULL
    assert out.tobytes() == ov.layout_coverage(edges_res, rows).tobytes()
    empty, _ = other.layout_edges(other_rows)                                 # a graph without edges: nothing is written
    assert lib.po_layout_coverage(other._h, empty._ptr, other_rows._ptr, None, None) == _lib.PO_OK
    assert len(other.layout_coverage(empty, other_rows)) == 0 and other.coverage_stats()["n_edges"] == 0
    assert len(layout.average_coverage(other, empty, other_rows)) == 0
    for r in (empty, other_rows):
        r.free()
    other.close()
    for ov, rows, edges_res in held:
        edges_res.free()
        rows.free()
        ov.close()
