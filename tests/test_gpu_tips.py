"""Tip removal + symmetry pass + isolated nodes on the device (po_layout_tips) and the node order of an edge result
(po_result_node_order) against the golden cases that the reference's own functions produced
(tests/golden/tips_cases.npz).  Exact integers throughout.  The direct cases of the golden file (graphs filled edge by
edge) have no GFA text; tests/test_tips_host_emulation.py runs the kernels on them."""
import numpy as np
import pytest

import golden_utils as gu
import reduce_utils as ru
import tips_utils as tu
from phasm_amd import layout
from phasm_amd.io import gfa
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

GOLDEN = tu.load_golden()
CASES = [c for c in GOLDEN["cases"] if not c.get("direct")]
STAT_KEYS = ("n_in_tip_edges", "n_out_tip_edges", "n_asymmetric", "n_isolated_nodes", "n_nodes", "n_candidates_in", "n_candidates_out")


def edge_array(e):
    return np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)


def edges_from_text(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(tu.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    return ov, edges_res


def check_tips(ov, in_res, L, B, rec, flags_key="flags", left_key="order_left"):
    """One application on ``in_res`` against its record; returns the kept result."""
    want = rec if flags_key == "flags" else rec["second"]
    before = edge_array(in_res.rows())
    order_before = in_res.node_order().tolist()
    kept_res, flags = ov.layout_tips(in_res, L, B, want_flags=True)
    st = ov.tips_stats()
    kept = edge_array(kept_res.rows())
    assert np.array_equal(flags[tu.by_uv(before)], ru.unpack_flags(rec[flags_key], len(before)))
    assert kept.tolist() == before[flags == 0].tolist()                     # the kept edges, in input order
    assert ru.edge_digest(ru.sort_edges(kept)) == want["kept_sha256"]
    assert (st["n_edges_in"], st["n_edges_out"]) == (want["n_in"], want["n_kept"])
    assert {k: st[k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}
    assert (st["n_rounds_in"] > 0) == (st["n_candidates_in"] > 0) and (st["n_rounds_out"] > 0) == (st["n_candidates_out"] > 0)
    assert max(st["n_rounds_in"], st["n_rounds_out"]) <= GOLDEN["branch_totals"]["max_rounds"]
    assert kept_res.node_order().tolist() == rec[left_key]
    assert edge_array(in_res.rows()).tolist() == before.tolist()            # the input stays as it was,
    assert in_res.node_order().tolist() == order_before                     # its node order too
    return kept_res


def check_case(case, ov, edges_res):
    assert edges_res.node_order().tolist() == case["order"]
    for r in case["results"]:
        if r["fuzz"] is None:
            in_res = edges_res                                              # tips on a stage-1 result
        else:
            in_res = ov.layout_reduce(edges_res, int(r["fuzz"]))            # ... on a reduce result
            assert in_res.node_order().tolist() == case["order"]
        kept_res = check_tips(ov, in_res, r["L"], r["B"], r)
        if "second" in r:                                                   # ... on their own result
            again = check_tips(ov, kept_res, r["second"]["L"], r["second"]["B"], r, "flags2", "order_left2")
            assert ov.tips_stats()["n_nodes"] == r["n_nodes"] - r["n_isolated_nodes"]   # isolated nodes are not counted twice
            again.free()
        kept_res.free()
        if in_res is not edges_res:
            in_res.free()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tips_from_gfa_text_equal_the_reference(case, tmp_path):
    ov, edges_res = edges_from_text(case, tmp_path)
    check_case(case, ov, edges_res)
    edges_res.free()
    ov.close()


LADDERS = [c for c in CASES if "reduce_case" in c and c["reduce_case"] in ("ladder_varlen", "ladder_cfg2_mini")]


@pytest.mark.parametrize("case", LADDERS, ids=[c["name"] for c in LADDERS])
def test_ladder_straight_from_overlap_rows_with_and_without_the_table(case, monkeypatch):
    """The rows of po_overlaps never leave HBM.  They come in the library's emission order, not the golden file's, and
    the node order follows the rows: the expectation is the node-order rule on these rows and the sequential
    statement in that order (both pinned by the goldens, tests/test_tips_oracle.py).  The adjacent path and the table
    (PHASM_LAYOUT_TABLE=1) give the same node order, flags and edges."""
    _, seqs, m, _ = gu.ladder_case(case["reduce_case"])
    ov = ExactOverlapper()
    for i in range(len(seqs) // 2):
        ov.add_sequence("read%d+" % i, seqs[2 * i])
        ov.add_sequence("read%d-" % i, seqs[2 * i + 1])
    res = ov.overlaps_result(m)
    r = res.rows()
    rows = np.stack([r[f] for f in r.dtype.names], 1).astype(np.int64).tolist()
    want_order = tu.node_order(rows, ov.lengths(), **case["params"])
    seen = []
    for table in (False, True):
        if table:
            monkeypatch.setenv("PHASM_LAYOUT_TABLE", "1")
        else:
            monkeypatch.delenv("PHASM_LAYOUT_TABLE", raising=False)
        edges_res, _ = ov.layout_edges(res, **case["params"])
        assert edges_res.node_order().tolist() == want_order
        assert ov.node_order_stats()["n_rows"] == len(res) and ov.node_order_stats()["ms_total"] > 0
        for fuzz in (None, 1000):
            in_res = edges_res if fuzz is None else ov.layout_reduce(edges_res, fuzz)
            e = edge_array(in_res.rows())
            kept_res, flags = ov.layout_tips(in_res, want_flags=True)
            want_flags, want_left, want = tu.remove_tips(e, want_order)
            st = ov.tips_stats()
            assert np.array_equal(flags, want_flags) and kept_res.node_order().tolist() == want_left
            assert edge_array(kept_res.rows()).tolist() == e[flags == 0].tolist()
            assert {k: st[k] for k in want} == want
            seen.append((table, fuzz, flags.tobytes(), kept_res.rows().tobytes()))
            kept_res.free()
            if in_res is not edges_res:
                in_res.free()
        edges_res.free()
    assert [x[2:] for x in seen[:2]] == [x[2:] for x in seen[2:]]
    res.free()
    ov.close()


def test_same_answer_twice_and_after_other_parameters_and_the_error_cases(tmp_path):
    case = next(c for c in CASES if c["name"].startswith("tangle_"))
    ov, edges_res = edges_from_text(case, tmp_path)
    seen = {}
    for prm in ((4, 5000), (4, 5000), (2, 2500), (0, 5000), (4, 5000), (7, 100000), (2, 2500), (2**32 - 1, 2**31 - 1), (4, -1)):
        kept, flags = ov.layout_tips(edges_res, *prm, want_flags=True)
        key = (flags.tobytes(), kept.rows().tobytes(), kept.node_order().tobytes())
        kept.free()
        assert seen.setdefault(prm, key) == key
    assert len({k[0] for k in seen.values()}) >= 3
    assert not any(np.frombuffer(seen[p][0], np.uint8).any() for p in ((0, 5000), (4, -1)))   # nothing is a tip then
    check_case(case, ov, edges_res)
    # a result that is no edge result, one of another handle, bad parameter values
    other = ExactOverlapper()
    other.add_segment("x", 10)
    rows = other.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    with pytest.raises(ValueError):
        other.layout_tips(rows)
    with pytest.raises(ValueError):
        other.layout_tips(edges_res)
    with pytest.raises(ValueError):
        rows.node_order()
    with pytest.raises(ValueError):
        ov.layout_tips(edges_res, -1)
    with pytest.raises(ValueError):
        ov.layout_tips(edges_res, 4, 2**31)
    empty, _ = other.layout_edges(rows)                                     # a graph without edges: x+ and x- are no nodes
    kept = other.layout_tips(empty)
    assert len(kept) == 0 and other.tips_stats()["n_nodes"] == 0 and kept.node_order().tolist() == []
    for r in (kept, empty, rows, edges_res):
        r.free()
    other.close()
    ov.close()


def test_layout_functions_and_cli(tmp_path):
    from phasm_amd import cli
    case = next(c for c in CASES if c["name"] == "reduced_line_109")
    text = tu.case_text(case)
    names, lengths, _ = gfa.read_gfa2_rows(text.splitlines(True))
    L = np.repeat(lengths, 2)
    p = tmp_path / "overlaps.gfa"
    p.write_text(text)
    rec = next(r for r in case["results"] if r["fuzz"] == 150)
    both = layout.layout_from_gfa(str(p), reduce=True, length_fuzz=150, tips=True, **case["params"])
    only_reduce = layout.layout_from_gfa(str(p), reduce=True, length_fuzz=150, **case["params"])
    assert only_reduce.tip_flags is None and only_reduce.tips_stats is None
    assert both.flags.tolist() == only_reduce.flags.tolist() and both.reduce_stats["n_edges_out"] == len(only_reduce.edges)
    red = edge_array(only_reduce.edges)
    assert np.array_equal(both.tip_flags[tu.by_uv(red)], ru.unpack_flags(rec["flags"], len(red)))
    assert edge_array(both.edges).tolist() == red[both.tip_flags == 0].tolist()
    assert both.tips_stats["n_isolated_nodes"] == rec["n_isolated_nodes"] > 0 and len(both.edges) == rec["n_kept"] < len(red)
    only_tips = layout.layout_from_gfa(str(p), tips=True, max_tip_len=2, max_tip_len_bases=2500, **case["params"])
    plain = layout.layout_from_gfa(str(p), **case["params"])
    assert only_tips.flags is None and len(only_tips.tip_flags) == len(plain.edges)
    assert edge_array(only_tips.edges).tolist() == edge_array(plain.edges)[only_tips.tip_flags == 0].tolist()
    # the CLI writes the same graph
    out0, out1, out2 = tmp_path / "g0.gfa", tmp_path / "g1.gfa", tmp_path / "g2.gfa"
    assert cli.main(["layout-edges", str(p), "--transitive-reduction", "-F", "150", "-o", str(out0)]) == 0
    assert cli.main(["layout-edges", str(p), "--transitive-reduction", "-F", "150", "-t", "9", "--max-tip-length-bases", "1", "-o", str(out1)]) == 0
    assert out0.read_bytes() == out1.read_bytes()                           # the two bounds alone change nothing
    assert cli.main(["layout-edges", str(p), "--transitive-reduction", "-F", "150", "--remove-tips", "-o", str(out2)]) == 0
    node = lambda n: names[n >> 1] + "+-"[n & 1]   # noqa: E731
    want = edge_array(both.edges).tolist()
    lines = out2.read_text().splitlines(True)
    e_lines = [l for l in lines if l.startswith("E\t")]
    s_lines = [l for l in lines if l.startswith("S\t")]
    assert lines[0] == "H\tVN:z:2.0\n" and len(lines) == 1 + len(s_lines) + len(e_lines)
    assert e_lines == [gfa.gfa_line("E", "*", node(u), node(v), w, int(L[u]), 0, o, "*") for u, v, w, o in want]
    used = sorted({n >> 1 for u, v, _, _ in want for n in (u, v)})
    assert s_lines == [gfa.gfa_line("S", names[i], int(lengths[i]), "*") for i in used]
    assert cli.main(["layout-edges", str(p), "--remove-tips", "-t", "2", "--max-tip-length-bases", "2500", "-o", str(out1)]) == 0
    assert len([l for l in out1.read_text().splitlines() if l.startswith("E\t")]) == len(only_tips.edges)
