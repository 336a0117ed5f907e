"""Diamond-tip removal on the device (po_layout_diamonds) and the whole graph-cleaning chain of `phasm layout` up to the
merging of paths (layout.clean_assembly_graph, ``layout-edges --clean``) against the golden applications that the
reference's own functions produced (tests/golden/diamond_cases.npz).  Exact integers throughout.  The direct cases of
the golden file (graphs filled edge by edge) have no GFA text; tests/test_diamond_host_emulation.py runs the kernels on
them."""
import ctypes
import logging

import numpy as np
import pytest

import diamond_utils as du
import golden_utils as gu
import reduce_utils as ru
import tips_utils as tu
from phasm_amd import _lib, layout
from phasm_amd.io import gfa
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

GOLDEN = du.load_golden()
CASES = [c for c in GOLDEN["cases"] if not c.get("direct")]
BY_NAME = {c["name"]: c for c in CASES}


def edge_array(e):
    return np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)


def edges_from_text(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(du.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    return ov, edges_res


def check_stats(st, want, max_rounds):
    assert {k: st[k] for k in du.STAT_KEYS} == {k: want[k] for k in du.STAT_KEYS}
    if want["n_candidates"]:
        assert 0 < st["n_rounds"] <= max_rounds
    else:
        assert st["n_rounds"] == 0


def check_diamonds(ov, in_res, rec):
    """One application on ``in_res`` against its record, and a second one on its own output against the restatement
    (which tests/test_diamond_oracle.py holds to the reference); returns the kept result and the flags."""
    before = edge_array(in_res.rows())
    order_before = in_res.node_order().tolist()
    assert order_before == rec["order_before"]
    kept_res, flags = ov.layout_diamonds(in_res, want_flags=True)
    st = ov.diamond_stats()
    kept = edge_array(kept_res.rows())
    assert np.array_equal(flags[tu.by_uv(before)], ru.unpack_flags(rec["flags"], len(before)))
    assert kept.tolist() == before[flags == 0].tolist()                     # the kept edges, in input order
    assert ru.edge_digest(ru.sort_edges(kept)) == rec["kept_sha256"]
    check_stats(st, {"n_edges_in": rec["n_in"], "n_edges_out": rec["n_kept"], "n_nodes": rec["n_nodes"],
                     "n_nodes_removed": 2 * rec["n_diamonds"], "n_candidates": rec["n_candidates"],
                     "n_diamonds": rec["n_diamonds"], "n_invalid": 0}, rec["rounds"])
    assert kept_res.node_order().tolist() == rec["order_left"]
    assert edge_array(in_res.rows()).tolist() == before.tolist()            # the input stays as it was,
    assert in_res.node_order().tolist() == order_before                     # its node order too
    want_flags, want_left, want = du.remove_diamond_tips(kept, rec["order_left"])
    _, want_rounds = du.remove_diamond_tips_rounds(kept, rec["order_left"])
    again, flags2 = ov.layout_diamonds(kept_res, want_flags=True)
    assert np.array_equal(flags2, want_flags) and again.node_order().tolist() == want_left
    assert edge_array(again.rows()).tolist() == kept[want_flags == 0].tolist()
    check_stats(ov.diamond_stats(), want, want_rounds)
    again.free()
    return kept_res, flags


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_diamonds_and_the_chain_from_gfa_text_equal_the_reference(case, tmp_path):
    ov, edges_res = edges_from_text(case, tmp_path)
    assert edges_res.node_order().tolist() == case["order"]
    rec_a, rec_b = case["results"]
    kept, _ = check_diamonds(ov, edges_res, rec_a)                          # (a) on the stage-1 result
    kept.free()
    ch = case["chain"]
    reduced, f0 = ov.layout_reduce(edges_res, ch["fuzz"], want_flags=True)
    tipped, f1 = ov.layout_tips(reduced, ch["L"], ch["B"], want_flags=True)
    kept, f2 = check_diamonds(ov, tipped, rec_b)                            # (b) after the reduction and the tips
    # the second tip block on the diamond result: it counts the nodes the diamonds isolated
    final, f3 = ov.layout_tips(kept, ch["L"], tu.DEFAULT_B, want_flags=True)
    st = ov.tips_stats()
    assert st["n_nodes"] == rec_b["n_nodes"] - 2 * rec_b["n_diamonds"]
    assert (st["n_in_tip_edges"] + st["n_out_tip_edges"], st["n_isolated_nodes"], st["n_asymmetric"], st["n_edges_out"]) == \
           (ch["n_tip_edges2"], ch["n_isolated_nodes2"], ch["n_asymmetric2"], ch["n_kept"])
    assert final.node_order().tolist() == ch["order_left"]
    assert ru.edge_digest(ru.sort_edges(edge_array(final.rows()))) == ch["kept_sha256"]
    s1 = edge_array(edges_res.rows())
    assert np.array_equal(du.compose_removed_by([f0, f1, f2, f3])[tu.by_uv(s1)], case["removed_by"])
    for r in (final, kept, tipped, reduced, edges_res):
        r.free()
    ov.close()


ENTRY = ["union_21_1", "reduced_stagger_1100", "reduced_hub_1024", "selfish_2", "reduced_ladder_varlen"]


def check_clean(got, case, s1):
    ch = case["chain"]
    assert np.array_equal(got.removed_by[tu.by_uv(s1)], case["removed_by"])
    assert edge_array(got.edges).tolist() == s1[got.removed_by == 0].tolist()
    assert ru.edge_digest(ru.sort_edges(edge_array(got.edges))) == ch["kept_sha256"]
    counts = du.chain_counts(got.clean_stats)
    assert counts == {k: ch[k] for k in counts}
    assert [st["n_edges_in"] for st in got.clean_stats] == [ch["n_stage1"]] + [st["n_edges_out"] for st in got.clean_stats[:3]]


@pytest.mark.parametrize("name", ENTRY)
def test_clean_assembly_graph_and_the_cli_equal_the_chain_record(name, tmp_path, caplog):
    from phasm_amd import cli
    case = BY_NAME[name]
    ch = case["chain"]
    ov, edges_res = edges_from_text(case, tmp_path)
    s1 = edge_array(edges_res.rows())
    got = layout.clean_assembly_graph(ov, edges_res)
    check_clean(got, case, s1)
    assert edge_array(edges_res.rows()).tolist() == s1.tolist() and edges_res.node_order().tolist() == case["order"]
    # stage (a) through the layout function; defaults leave the other fields alone
    a = layout.remove_diamond_tips(ov, edges_res)
    rec_a = case["results"][0]
    assert np.array_equal(a.diamond_flags[tu.by_uv(s1)], ru.unpack_flags(rec_a["flags"], len(s1)))
    assert a.diamond_stats["n_diamonds"] == rec_a["n_diamonds"] and a.removed_by is None and a.tip_flags is None and a.flags is None
    edges_res.free()
    ov.close()
    p = tmp_path / "in.gfa"
    params = {k: v for k, v in case["params"].items()}
    from_file = layout.layout_from_gfa(str(p), clean=True, **params)
    check_clean(from_file, case, s1)
    plain = layout.layout_from_gfa(str(p), **params)
    assert plain.removed_by is None and plain.clean_stats is None and plain.diamond_flags is None and plain.diamond_stats is None
    # the CLI writes the same edges and logs the reference's lines with the recorded numbers
    argv = ["-l", str(params["min_read_length"]), "-s", str(params["min_overlap_length"]), "-a", str(params["max_overhang_abs"]),
            "-r", repr(params["max_overhang_rel"])]
    names, lengths, _ = gfa.read_gfa2_rows(du.case_text(case).splitlines(True))
    L = np.repeat(lengths, 2)
    node = lambda n: names[n >> 1] + "+-"[n & 1]   # noqa: E731
    out1, out2 = tmp_path / "clean.gfa", tmp_path / "diamonds.gfa"
    with caplog.at_level(logging.INFO, logger=cli.logger.name):
        assert cli.main(["layout-edges", str(p), "--clean", "-o", str(out1)] + argv) == 0
    e_lines = [l for l in out1.read_text().splitlines(True) if l.startswith("E\t")]
    assert e_lines == [gfa.gfa_line("E", "*", node(u), node(v), w, int(L[u]), 0, o, "*") for u, v, w, o in edge_array(got.edges).tolist()]
    msgs = [r.getMessage() for r in caplog.records]
    st0, st1 = got.clean_stats[:2]
    assert "Removing %d transitive edges..." % ch["n_transitive"] in msgs
    assert st0["n_asymmetric"] + st1["n_asymmetric"] == ch["n_asymmetric"]
    assert "Removed %d tip edges, %d isolated nodes, %d asymmetric edges." % (ch["n_tip_edges"], ch["n_isolated_nodes"], st1["n_asymmetric"]) in msgs
    assert "Removed %d diamond tips" % ch["n_diamonds"] in msgs
    at = msgs.index("Removing tips (stage 2)...")
    assert msgs.index("Removed %d diamond tips" % ch["n_diamonds"]) < at
    assert msgs[at + 1] == "Removed %d tip edges, %d isolated nodes, %d asymmetric edges." % (
        ch["n_tip_edges2"], ch["n_isolated_nodes2"], ch["n_asymmetric2"])
    # --remove-diamond-tips alone is stage (a)
    assert cli.main(["layout-edges", str(p), "--remove-diamond-tips", "-o", str(out2)] + argv) == 0
    e_lines = [l for l in out2.read_text().splitlines(True) if l.startswith("E\t")]
    assert e_lines == [gfa.gfa_line("E", "*", node(u), node(v), w, int(L[u]), 0, o, "*") for u, v, w, o in s1[a.diamond_flags == 0].tolist()]
    assert len(e_lines) == rec_a["n_kept"]


LADDERS = [c for c in CASES if c.get("reduce_case") in ("ladder_varlen", "ladder_cfg2_mini")]


@pytest.mark.parametrize("case", LADDERS, ids=[c["name"] for c in LADDERS])
def test_ladder_straight_from_overlap_rows_with_and_without_the_table(case, monkeypatch):
    """The rows of po_overlaps never leave HBM.  They come in the library's emission order, not the golden file's, and the
    node order follows the rows: the expectation is the sequential statement in the node order the device reports (which
    tests/test_gpu_tips.py holds to the node-order rule).  The adjacent path and the table (PHASM_LAYOUT_TABLE=1) give
    the same flags, edges and node orders."""
    _, seqs, m, _ = gu.ladder_case(case["reduce_case"])
    ov = ExactOverlapper()
    for i in range(len(seqs) // 2):
        ov.add_sequence("read%d+" % i, seqs[2 * i])
        ov.add_sequence("read%d-" % i, seqs[2 * i + 1])
    res = ov.overlaps_result(m)
    seen = []
    for table in (False, True):
        if table:
            monkeypatch.setenv("PHASM_LAYOUT_TABLE", "1")
        else:
            monkeypatch.delenv("PHASM_LAYOUT_TABLE", raising=False)
        edges_res, _ = ov.layout_edges(res, **case["params"])
        reduced = ov.layout_reduce(edges_res, du.STAGE_FUZZ)
        tipped = ov.layout_tips(reduced)
        for in_res in (edges_res, tipped):
            e, order = edge_array(in_res.rows()), in_res.node_order().tolist()
            want_flags, want_left, want = du.remove_diamond_tips(e, order)
            kept, flags = ov.layout_diamonds(in_res, want_flags=True)
            st = ov.diamond_stats()
            assert np.array_equal(flags, want_flags) and kept.node_order().tolist() == want_left
            assert edge_array(kept.rows()).tolist() == e[flags == 0].tolist()
            assert {k: st[k] for k in want} == want
            seen.append((table, flags.tobytes(), kept.rows().tobytes(), kept.node_order().tobytes()))
            kept.free()
        for r in (tipped, reduced, edges_res):
            r.free()
    assert [x[1:] for x in seen[:2]] == [x[1:] for x in seen[2:]]
    res.free()
    ov.close()


def test_interleaved_calls_on_one_handle_and_the_error_cases(tmp_path):
    """Diamonds and tips share their workspaces on the handle: five rounds of both, on two graphs, give the same bytes."""
    held = []
    for name in ("reduced_hub_1025", "reduced_stagger_1100"):
        d = tmp_path / name
        d.mkdir()
        ov, edges_res = edges_from_text(BY_NAME[name], d)
        reduced = ov.layout_reduce(edges_res, du.STAGE_FUZZ)
        held.append((ov, edges_res, reduced))
    for ov, edges_res, reduced in held:
        seen = set()
        for _ in range(5):
            tipped, f1 = ov.layout_tips(reduced, want_flags=True)
            kept, f2 = ov.layout_diamonds(tipped, want_flags=True)
            a, fa = ov.layout_diamonds(edges_res, want_flags=True)
            final, f3 = ov.layout_tips(kept, du.STAGE_L, tu.DEFAULT_B, want_flags=True)
            seen.add((f1.tobytes(), f2.tobytes(), fa.tobytes(), f3.tobytes(), kept.rows().tobytes(), kept.node_order().tobytes(),
                      a.rows().tobytes(), a.node_order().tobytes(), final.rows().tobytes(), final.node_order().tobytes()))
            for r in (final, a, kept, tipped):
                r.free()
        assert len(seen) == 1
        assert np.frombuffer(next(iter(seen))[1], np.uint8).any()
    ov, edges_res, _ = held[0]
    # a result that is no edge result, one of another handle, a non-zero reserved word
    other = ExactOverlapper()
    other.add_segment("x", 10)
    rows = other.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    with pytest.raises(ValueError):
        other.layout_diamonds(rows)
    with pytest.raises(ValueError):
        other.layout_diamonds(edges_res)
    lib = _lib.load()
    for reserved, want in ((1, _lib.PO_ERR_INVALID), (0, _lib.PO_OK)):
        r = ctypes.c_void_p()
        prm = _lib.PoDiamondParams(reserved)
        assert lib.po_layout_diamonds(ov._h, edges_res._ptr, ctypes.byref(prm), None, ctypes.byref(r)) == want
        assert bool(r.value) == (want == _lib.PO_OK)
        if r.value:
            lib.po_result_free(r)
    r = ctypes.c_void_p()
    assert lib.po_layout_diamonds(ov._h, edges_res._ptr, None, None, ctypes.byref(r)) == _lib.PO_OK      # params may be NULL
    lib.po_result_free(r)
    empty, _ = other.layout_edges(rows)                                     # a graph without edges: x+ and x- are no nodes
    kept = other.layout_diamonds(empty)
    st = other.diamond_stats()
    assert len(kept) == 0 and kept.node_order().tolist() == [] and (st["n_nodes"], st["n_candidates"], st["n_rounds"]) == (0, 0, 0)
    for r in (kept, empty, rows):
        r.free()
    other.close()
    for ov, edges_res, reduced in held:
        reduced.free()
        edges_res.free()
        ov.close()
