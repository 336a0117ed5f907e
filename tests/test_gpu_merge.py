"""Merging of unambiguous paths on the device (po_layout_merge) and the graph file of `phasm layout`
(layout.merge_unambiguous_paths, ``merge=True``, ``layout-edges --merge``) against the golden applications that the
reference's own merge_unambiguous_paths and gfa2_write_graph produced (tests/golden/merge_cases.npz).  Exact integers
throughout.  The direct cases of the golden file (graphs filled edge by edge: long paths, pure cycles, the overflow) have
no GFA text; tests/test_merge_host_emulation.py runs the kernels on them."""
import ctypes
import logging
import math

import numpy as np
import pytest

import diamond_utils as du
import golden_utils as gu
import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu
from phasm_amd import _lib, layout
from phasm_amd.io import gfa
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

GOLDEN = mu.load_golden()
CASES = [c for c in GOLDEN["cases"] if not c.get("direct")]
BY_NAME = {c["name"]: c for c in CASES}


def edge_array(e):
    return np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)


def edges_from_text(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(mu.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    return ov, edges_res


def cleaned(ov, edges_res):
    """The chain at the CLI defaults as four device calls; returns the last result."""
    cur = edges_res
    for call in (lambda r: ov.layout_reduce(r, du.STAGE_FUZZ), lambda r: ov.layout_tips(r, du.STAGE_L, du.STAGE_B),
                 ov.layout_diamonds, lambda r: ov.layout_tips(r, du.STAGE_L, tu.DEFAULT_B)):
        nxt = call(cur)
        if cur is not edges_res:
            cur.free()
        cur = nxt
    return cur


def check_stats(st, rec):
    assert {k: st[k] for k in mu.STAT_KEYS} == {k: rec[k] for k in mu.STAT_KEYS}
    assert st["n_rounds"] <= math.ceil(math.log2(max(st["n_nodes"], 1))) + 1
    assert (st["n_rounds"] > 0) == (rec["n_merged"] > 0) and st["n_rounds"] <= rec["rounds"]


def check_merge(ov, in_res, rec):
    """One application on ``in_res`` against its record; returns the merged result's arrays."""
    before = edge_array(in_res.rows())
    order_before = in_res.node_order().tolist()
    assert order_before == rec["order_before"] and len(ov) == rec["n_ids"]
    merged, flags = ov.layout_merge(in_res, want_flags=True)
    st = ov.merge_stats()
    got = edge_array(merged.rows())
    assert np.array_equal(flags[tu.by_uv(before)], ru.unpack_flags(rec["flags"], len(before)))
    want = mu.merge_paths(before, order_before, ov.lengths().tolist(), len(ov))
    assert got.tolist() == want["edges"].tolist()                           # the kept edges, renamed, in input order
    assert ru.edge_digest(ru.sort_edges(got)) == rec["kept_sha256"]
    offsets, members, prefix, lengths = merged.merged_paths()
    for a, key in ((offsets, "offsets"), (members, "members"), (prefix, "prefix"), (lengths, "lengths")):
        assert a.tolist() == rec[key].tolist(), key
    order = merged.node_order().tolist()
    assert order == du.minus(order_before, rec["members"].tolist()) + [rec["n_ids"] + k for k in range(rec["n_merged"])]
    check_stats(st, rec)
    assert edge_array(in_res.rows()).tolist() == before.tolist()            # the input stays as it was,
    assert in_res.node_order().tolist() == order_before                     # its node order too
    for call in (ov.layout_merge, ov.layout_diamonds, ov.layout_tips, ov.layout_reduce):
        with pytest.raises(ValueError):                                     # a merged graph is not cleaned or merged again
            call(merged)
    merged.free()
    return got, flags


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merge_from_gfa_text_equals_the_reference(case, tmp_path):
    ov, edges_res = edges_from_text(case, tmp_path)
    assert edges_res.node_order().tolist() == case["order"]
    rec_a, rec_b = case["results"]
    check_merge(ov, edges_res, rec_a)                                       # (a) on the stage-1 result
    final = cleaned(ov, edges_res)
    check_merge(ov, final, rec_b)                                           # (b) after the whole chain
    final.free()
    edges_res.free()
    ov.close()


ENTRY = ["union_21_1", "reduced_hub_1024", "selfish_2", "reduced_line_101", "ring_40", "lasso_70_6"]


def same_merge(a, b):
    assert a.edges.tobytes() == b.edges.tobytes() and a.merge_flags.tobytes() == b.merge_flags.tobytes()
    assert a.node_order.tolist() == b.node_order.tolist()
    assert all(x.tolist() == y.tolist() for x, y in zip(a.merged_paths, b.merged_paths))
    assert {k: a.merge_stats[k] for k in mu.STAT_KEYS} == {k: b.merge_stats[k] for k in mu.STAT_KEYS}


@pytest.mark.parametrize("name", ENTRY)
def test_the_entry_points_and_the_cli_write_the_file_of_the_reference(name, tmp_path, caplog):
    from phasm_amd import cli
    case = BY_NAME[name]
    rec = case["results"][1]
    ov, edges_res = edges_from_text(case, tmp_path)
    final = cleaned(ov, edges_res)
    direct = layout.merge_unambiguous_paths(ov, final)
    final.free()
    chained = layout.clean_assembly_graph(ov, edges_res, merge=True)
    plain = layout.clean_assembly_graph(ov, edges_res)
    edges_res.free()
    ov.close()
    same_merge(direct, chained)
    assert direct.removed_by is None and chained.removed_by.tolist() == plain.removed_by.tolist()
    assert plain.merge_flags is None and plain.merged_paths is None and plain.merge_stats is None
    assert len(chained.merge_flags) == len(plain.edges) == int((chained.removed_by == 0).sum())
    assert {k: chained.merge_stats[k] for k in mu.STAT_KEYS} == {k: rec[k] for k in mu.STAT_KEYS}
    p = tmp_path / "in.gfa"
    params = dict(case["params"])
    same_merge(layout.layout_from_gfa(str(p), merge=True, **params), chained)
    assert layout.layout_from_gfa(str(p), clean=True, **params).edges.tobytes() == plain.edges.tobytes()
    # the CLI writes what gfa2_write_graph wrote: H / S / F lines in order, E lines as a sorted list
    argv = ["-l", str(params["min_read_length"]), "-s", str(params["min_overlap_length"]), "-a", str(params["max_overhang_abs"]),
            "-r", repr(params["max_overhang_rel"])]
    out1, out2, out3 = tmp_path / "merge.gfa", tmp_path / "clean.gfa", tmp_path / "clean_again.gfa"
    with caplog.at_level(logging.INFO, logger=cli.logger.name):
        assert cli.main(["layout-edges", str(p), "--merge", "-o", str(out1)] + argv) == 0
    lines = out1.read_text().splitlines(True)
    head = lines[:rec["n_hsf_lines"]]
    assert all(l[0] in "HSF" for l in head) and all(l[0] == "E" for l in lines[len(head):])
    assert mu.lines_digest(head) == rec["hsf_sha256"]
    assert mu.lines_digest(sorted(lines[len(head):])) == rec["e_sorted_sha256"]
    msgs = [r.getMessage() for r in caplog.records]
    at = msgs.index("Merging unambiguous paths...")
    assert msgs[at + 1] == "Merged %d nodes." % rec["n_nodes_merged"] and "Removing tips (stage 2)..." in msgs[:at]
    # without --merge: exactly what --clean writes, with the same E lines as the library's clean result
    assert cli.main(["layout-edges", str(p), "--clean", "-o", str(out2)] + argv) == 0
    assert cli.main(["layout-edges", str(p), "--clean", "-o", str(out3)] + argv) == 0
    assert out2.read_bytes() == out3.read_bytes() and b"\nF\t" not in out2.read_bytes() and b"merged" not in out2.read_bytes()
    names, lengths, _ = gfa.read_gfa2_rows(mu.case_text(case).splitlines(True))
    L = np.repeat(lengths, 2)
    node = lambda n: names[n >> 1] + "+-"[n & 1]   # noqa: E731
    # the whole file, byte for byte, as the command builds it without the merge: the header, one S line per read that
    # still has an edge in the order of the input's S lines, the E lines of the cleaned graph in its own order
    pe = edge_array(plain.edges)
    used = sorted(set((pe[:, 0] >> 1).tolist()) | set((pe[:, 1] >> 1).tolist()))
    want = [gfa.gfa_header()] + [gfa.gfa_line("S", names[i], int(lengths[i]), "*") for i in used] + \
           [gfa.gfa_line("E", "*", node(u), node(v), w, int(L[u]), 0, o, "*") for u, v, w, o in pe.tolist()]
    assert out2.read_text() == "".join(want)


LADDERS = [c for c in CASES if c.get("reduce_case") in ("ladder_varlen", "ladder_cfg2_mini")]


@pytest.mark.parametrize("case", LADDERS, ids=[c["name"] for c in LADDERS])
def test_ladder_straight_from_overlap_rows_with_and_without_the_table(case, monkeypatch):
    """The rows of po_overlaps never leave HBM.  They come in the library's emission order, not the golden file's, and the
    node order follows the rows: the expectation is the plain statement in the node order the device reports.  The
    adjacent path and the table (PHASM_LAYOUT_TABLE=1) give the same bytes."""
    _, seqs, m, _ = gu.ladder_case(case["reduce_case"])
    ov = ExactOverlapper()
    for i in range(len(seqs) // 2):
        ov.add_sequence("read%d+" % i, seqs[2 * i])
        ov.add_sequence("read%d-" % i, seqs[2 * i + 1])
    res = ov.overlaps_result(m)
    L = ov.lengths().tolist()
    seen = []
    for table in (False, True):
        if table:
            monkeypatch.setenv("PHASM_LAYOUT_TABLE", "1")
        else:
            monkeypatch.delenv("PHASM_LAYOUT_TABLE", raising=False)
        edges_res, _ = ov.layout_edges(res, **case["params"])
        final = cleaned(ov, edges_res)
        for in_res in (edges_res, final):
            e, order = edge_array(in_res.rows()), in_res.node_order().tolist()
            want = mu.merge_paths(e, order, L, len(ov))
            merged, flags = ov.layout_merge(in_res, want_flags=True)
            st = ov.merge_stats()
            assert np.array_equal(flags, want["flags"]) and merged.node_order().tolist() == want["order"]
            assert edge_array(merged.rows()).tolist() == want["edges"].tolist()
            tables = merged.merged_paths()
            for a, key in zip(tables, ("offsets", "members", "prefix", "lengths")):
                assert a.tolist() == want[key].tolist(), key
            assert {k: st[k] for k in mu.STAT_KEYS} == {k: want["stats"][k] for k in mu.STAT_KEYS}
            seen.append((flags.tobytes(), merged.rows().tobytes(), merged.node_order().tobytes()) + tuple(a.tobytes() for a in tables))
            merged.free()
        final.free()
        edges_res.free()
    assert seen[:2] == seen[2:]
    assert any(np.frombuffer(x[0], np.uint8).any() for x in seen)
    res.free()
    ov.close()


def test_interleaved_calls_on_one_handle_and_the_error_cases(tmp_path):
    """The workspaces of the merge live on the handle beside those of the tips and diamonds: merge, tips, diamonds and
    merge again, five times over, on two graphs, give the same bytes."""
    held = []
    for name in ("reduced_hub_1025", "lasso_70_6"):
        d = tmp_path / name
        d.mkdir()
        ov, edges_res = edges_from_text(BY_NAME[name], d)
        reduced = ov.layout_reduce(edges_res, du.STAGE_FUZZ)
        held.append((ov, edges_res, reduced))
    for ov, edges_res, reduced in held:
        seen = set()
        for _ in range(5):
            m1, f1 = ov.layout_merge(reduced, want_flags=True)
            tipped = ov.layout_tips(reduced)
            kept = ov.layout_diamonds(tipped)
            m2, f2 = ov.layout_merge(kept, want_flags=True)
            m3, f3 = ov.layout_merge(edges_res, want_flags=True)
            seen.add(tuple(x.tobytes() for m, f in ((m1, f1), (m2, f2), (m3, f3))
                           for x in (f, m.rows(), m.node_order()) + m.merged_paths()))
            for r in (m3, m2, kept, tipped, m1):
                r.free()
        assert len(seen) == 1
        assert np.frombuffer(next(iter(seen))[0], np.uint8).any()
    ov, edges_res, _ = held[0]
    # a result that is no edge result, one of another handle, a non-zero reserved word
    other = ExactOverlapper()
    other.add_segment("x", 10)
    rows = other.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    with pytest.raises(ValueError):
        other.layout_merge(rows)
    with pytest.raises(ValueError):
        other.layout_merge(edges_res)
    with pytest.raises(ValueError):
        edges_res.merged_paths()                                            # no merged graph
    lib = _lib.load()
    for reserved, want in ((1, _lib.PO_ERR_INVALID), (0, _lib.PO_OK)):
        r = ctypes.c_void_p()
        prm = _lib.PoMergeParams(reserved)
        assert lib.po_layout_merge(ov._h, edges_res._ptr, ctypes.byref(prm), None, ctypes.byref(r)) == want
        assert bool(r.value) == (want == _lib.PO_OK)
        if r.value:
            lib.po_result_free(r)
    r = ctypes.c_void_p()
    assert lib.po_layout_merge(ov._h, edges_res._ptr, None, None, ctypes.byref(r)) == _lib.PO_OK          # params may be NULL
    lib.po_result_free(r)
    empty, _ = other.layout_edges(rows)                                     # a graph without edges: x+ and x- are no nodes
    merged = other.layout_merge(empty)
    st = other.merge_stats()
    assert len(merged) == 0 and merged.node_order().tolist() == [] and (st["n_nodes"], st["n_merged"], st["n_rounds"]) == (0, 0, 0)
    assert [a.tolist() for a in merged.merged_paths()] == [[0], [], [], []]
    for r in (merged, empty, rows):
        r.free()
    other.close()
    for ov, edges_res, reduced in held:
        reduced.free()
        edges_res.free()
        ov.close()
