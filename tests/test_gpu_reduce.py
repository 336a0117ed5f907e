"""Transitive reduction + symmetry pass on the device (po_layout_reduce) against the golden cases that the reference's
own functions produced (tests/golden/reduce_cases.npz), and -- where no golden can reach -- against the plain
statement of the contract (tests/reduce_utils.py).  Exact integers throughout."""
import io
import json
import os

import numpy as np
import pytest

import checker as ck   # stage-1 expectations come from the checker process, as in tests/test_gpu_layout.py
import golden_utils as gu
import layout_utils as lu
import reduce_utils as ru
from phasm_amd import layout, synth
from phasm_amd.io import gfa
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

GOLDEN = ru.load_golden()
CASES = GOLDEN["cases"]
LADDERS = [c for c in CASES if "ladder" in c and c["shuffle_seed"] is None]


def edge_array(e):
    return np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)


def by_uv(arr):
    return np.lexsort((arr[:, 1], arr[:, 0])) if len(arr) else np.empty(0, dtype=np.int64)


def check_against_golden(case, ov, edges_res, fuzzes=None):
    """Stage-1 edges == the reference's build_assembly_graph (attributes included); per fuzz: flags, kept edges and
    stats == the reference's remove_transitive_edges / make_symmetric.  One edges result serves every fuzz."""
    s1 = edge_array(edges_res.rows())
    order = by_uv(s1)
    assert len(s1) == case["n_stage1"]
    want1 = ru.case_stage1(case)
    if want1 is None:
        assert ru.edge_digest(s1[order]) == case["stage1_sha256"]
    else:
        assert s1[order].tolist() == ru.sort_edges(want1).tolist()
    for fuzz in (fuzzes or case["results"]):
        exp = case["results"][str(fuzz)]
        kept_res, flags = ov.layout_reduce(edges_res, int(fuzz), want_flags=True)
        kept = edge_array(kept_res.rows())
        kept_res.free()
        st = ov.reduce_stats()
        assert np.array_equal(flags[order], ru.unpack_flags(exp["flags_by_uv"], len(s1))), (case["name"], fuzz)
        assert kept.tolist() == s1[flags == 0].tolist()                       # the kept edges, in stage-1 order
        assert ru.edge_digest(ru.sort_edges(kept)) == exp["kept_sha256"]
        if "kept" in exp:
            assert ru.sort_edges(kept).tolist() == exp["kept"]
        assert (st["n_edges_in"], st["n_transitive"], st["n_asymmetric"], st["n_edges_out"]) == \
               (len(s1), exp["n_transitive"], exp["n_asymmetric"], exp["n_kept"])
        assert st["max_out_degree"] == (int(np.bincount(s1[:, 0]).max()) if len(s1) else 0)
        assert edge_array(edges_res.rows()).tolist() == s1.tolist()           # the input stays as it was
    return s1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reduce_from_gfa_text_equals_the_reference(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(ru.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    s1 = check_against_golden(case, ov, edges_res)
    assert ov.reduce_stats()["max_out_degree"] == GOLDEN["max_out_degree"][case["name"]]   # (5200, 1024, 1025, ...: as recorded)
    edges_res.free()
    ov.close()
    assert len(s1) == case["n_stage1"]


@pytest.mark.parametrize("case", LADDERS, ids=[c["name"] for c in LADDERS])
def test_ladders_straight_from_overlap_rows_with_and_without_the_table(case, monkeypatch):
    """The rows of po_overlaps never leave HBM.  Without the table the emission order is the edges' rank, with it
    (PHASM_LAYOUT_TABLE=1) the recorded first writer row: both give the reference's answer."""
    _, seqs, m, _ = gu.ladder_case(case["ladder"])
    ov = ExactOverlapper()
    for i in range(len(seqs) // 2):
        ov.add_sequence("read%d+" % i, seqs[2 * i])
        ov.add_sequence("read%d-" % i, seqs[2 * i + 1])
    res = ov.overlaps_result(m)
    for table in (False, True):
        if table:
            monkeypatch.setenv("PHASM_LAYOUT_TABLE", "1")
        else:
            monkeypatch.delenv("PHASM_LAYOUT_TABLE", raising=False)
        edges_res, _ = ov.layout_edges(res, **case["params"])
        check_against_golden(case, ov, edges_res)
        edges_res.free()
    res.free()
    ov.close()


def test_same_answer_twice_and_after_another_fuzz(tmp_path):
    case = next(c for c in CASES if c["name"] == "line_108")
    p = tmp_path / "in.gfa"
    p.write_text(ru.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    seen = {}
    for fuzz in (0, 0, 1000, 0, 150, 1000, 1000000, 150):
        kept, flags = ov.layout_reduce(edges_res, fuzz, want_flags=True)
        key = (flags.tobytes(), kept.rows().tobytes())
        kept.free()
        assert seen.setdefault(fuzz, key) == key
    assert len({k[0] for k in seen.values()}) == 4               # this case tells the four values apart
    check_against_golden(case, ov, edges_res)
    # a result that is not a po_layout_edges result, and one of another handle
    with pytest.raises(ValueError):
        ov.layout_reduce(rows)
    other = ExactOverlapper()
    other.add_segment("x", 10)
    with pytest.raises(ValueError):
        other.layout_reduce(edges_res)
    kept = ov.layout_reduce(edges_res, 150)
    again = ov.layout_reduce(kept, 150)                          # a kept result is an edge result like its input
    assert len(again) <= len(kept)
    for r in (again, kept, edges_res, rows):
        r.free()
    other.close()
    ov.close()


def edges_from_text(case, tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(ru.case_text(case))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    return ov, edges_res


SECOND_CASES = sorted({r["case"] for r in GOLDEN["second_pass"]}, key=[c["name"] for c in CASES].index)


@pytest.mark.parametrize("name", SECOND_CASES)
def test_reducing_a_kept_result_equals_the_reference_second_pass(name, tmp_path):
    """Reduced again, a kept result gives what the reference's three calls give on the graph their first run left,
    flag for flag.  Only tie_8 makes that depend on the hidden rank the kept result carries (k_reduce_emit): see
    test_a_second_pass_depends_on_the_rank_the_first_hands_on in tests/test_reduce_oracle.py."""
    case = next(c for c in CASES if c["name"] == name)
    ov, edges_res = edges_from_text(case, tmp_path)
    for rec in (r for r in GOLDEN["second_pass"] if r["case"] == name):
        kept_res, flags = ov.layout_reduce(edges_res, rec["fuzz"], want_flags=True)
        kept = edge_array(kept_res.rows())
        assert np.array_equal(flags[by_uv(edge_array(edges_res.rows()))],
                              ru.unpack_flags(case["results"][str(rec["fuzz"])]["flags_by_uv"], case["n_stage1"]))
        assert len(kept) == rec["n_in"]
        again_res, flags2 = ov.layout_reduce(kept_res, rec["fuzz2"], want_flags=True)
        again = edge_array(again_res.rows())
        st = ov.reduce_stats()
        assert np.array_equal(flags2[by_uv(kept)], ru.unpack_flags(rec["flags_by_uv"], len(kept))), (name, rec["fuzz"], rec["fuzz2"])
        assert again.tolist() == kept[flags2 == 0].tolist()
        assert ru.edge_digest(ru.sort_edges(again)) == rec["kept_sha256"]
        assert (st["n_edges_in"], st["n_transitive"], st["n_asymmetric"], st["n_edges_out"]) == \
               (rec["n_in"], rec["n_transitive"], rec["n_asymmetric"], rec["n_kept"])
        assert edge_array(kept_res.rows()).tolist() == kept.tolist()
        again_res.free()
        kept_res.free()
    edges_res.free()
    ov.close()


@pytest.mark.parametrize("name", ["dense_600", "stagger_1100", "hub_1025"])
def test_same_bytes_from_five_calls_between_calls_with_another_fuzz(name, tmp_path):
    """Out-degrees in the hundreds and above 1024: k_reduce_scatter's atomics hand out the slots of a long list in a
    new order every call, and many lanes store into one state array at once; neither may show in the answer.  From
    the second call on the global state workspace of the nodes above 1024 out-edges holds what the call before left
    (on a fresh handle it holds anything), so a state that a call does not set again shows here."""
    case = next(c for c in CASES if c["name"] == name)
    fuzz, other = (int(f) for f in list(case["results"])[:2])
    ov, edges_res = edges_from_text(case, tmp_path)
    seen = {}
    for f in (fuzz, other) * 5:
        kept, flags = ov.layout_reduce(edges_res, f, want_flags=True)
        key = (flags.tobytes(), kept.rows().tobytes())
        kept.free()
        assert seen.setdefault(f, key) == key
    assert seen[fuzz][0] != seen[other][0] or name.startswith("hub")    # (the hubs' two values give the same flags)
    s1 = edge_array(edges_res.rows())
    for f in (fuzz, other):
        got = np.frombuffer(seen[f][0], dtype=np.uint8)
        assert np.array_equal(got[by_uv(s1)], ru.unpack_flags(case["results"][str(f)]["flags_by_uv"], len(s1)))
    edges_res.free()
    ov.close()


def test_cli_with_and_without_transitive_reduction(tmp_path):
    from phasm_amd import cli
    case = next(c for c in CASES if c["name"] == "line_105")
    text = ru.case_text(case)
    names, lengths, _ = gfa.read_gfa2_rows(text.splitlines(True))
    L = np.repeat(lengths, 2)
    p = tmp_path / "overlaps.gfa"
    p.write_text(text)
    plain, plain2, reduced = tmp_path / "g0.gfa", tmp_path / "g1.gfa", tmp_path / "g2.gfa"
    assert cli.main(["layout-edges", str(p), "-o", str(plain)]) == 0
    assert cli.main(["layout-edges", str(p), "-F", "150", "-o", str(plain2)]) == 0          # -F alone changes nothing
    assert plain.read_bytes() == plain2.read_bytes()
    assert cli.main(["layout-edges", str(p), "--transitive-reduction", "-F", "150", "-o", str(reduced)]) == 0
    node = lambda n: names[n >> 1] + "+-"[n & 1]
    want = case["results"]["150"]["kept"]
    lines = reduced.read_text().splitlines(True)
    assert lines[0] == "H\tVN:z:2.0\n"
    e_lines = [l for l in lines if l.startswith("E\t")]
    s_lines = [l for l in lines if l.startswith("S\t")]
    assert len(lines) == 1 + len(s_lines) + len(e_lines)
    assert sorted(e_lines) == sorted(gfa.gfa_line("E", "*", node(u), node(v), w, int(L[u]), 0, o, "*") for u, v, w, o in want)
    used = sorted({n >> 1 for u, v, _, _ in want for n in (u, v)})
    assert s_lines == [gfa.gfa_line("S", names[i], int(lengths[i]), "*") for i in used]
    assert len(e_lines) < len([l for l in plain.read_text().splitlines() if l.startswith("E\t")])
    # the default fuzz is the reference's 1000
    assert cli.main(["layout-edges", str(p), "--transitive-reduction", "-o", str(plain2)]) == 0
    assert len([l for l in plain2.read_text().splitlines() if l.startswith("E\t")]) == case["results"]["1000"]["n_kept"]


def test_layout_from_daligner_with_reduce():
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "daligner_cases.json")))
    usable = [c for c in d["cases"] if "ok" in c["gfa"] and c["name"] not in ("no_reads", "trace_empty_list")]
    params = dict(layout.DEFAULTS, max_overhang_abs=20, max_overhang_rel=0.3)
    n_edges = 0
    for case in usable:
        plain = layout.layout_from_daligner(io.StringIO(case["db"]), io.StringIO(case["las"]), case["translations"], **params)
        assert plain.flags is None
        names, lengths, rows = gfa.read_gfa2_rows(io.StringIO(case["gfa"]["ok"]))
        want1 = ck.layout_sequential([tuple(r) for r in rows.tolist()], lu.node_lengths(lengths.tolist()), **params)["edges"]
        s1 = np.array([[u, v, w, o] for (u, v), (w, o) in want1.items()], dtype=np.int64).reshape(-1, 4)   # insertion order
        for fuzz in (1000, 5):
            got = layout.layout_from_daligner(io.StringIO(case["db"]), io.StringIO(case["las"]), case["translations"],
                                              reduce=True, length_fuzz=fuzz, **params)
            want_flags = ru.reduce_edges(s1, fuzz)
            assert ru.sort_edges(edge_array(got.edges)).tolist() == ru.sort_edges(s1[want_flags == 0]).tolist()
            g1 = edge_array(plain.edges)
            assert np.array_equal(got.flags[by_uv(g1)], want_flags[by_uv(s1)])
            assert got.reduce_stats["n_edges_out"] == len(got.edges) and got.contained.tolist() == plain.contained.tolist()
        n_edges += len(s1)
    assert n_edges > 20


@pytest.mark.timeout(1500, method="thread")
def test_full_config_2_sampled_nodes_and_every_edge():
    """100 000 nodes, about 6.9 M stage-1 edges.  The flags of ALL out-edges of 2 000 seeded nodes equal the contract
    run on their 2-hop neighbourhoods; for EVERY edge the symmetry rule holds; kept = flag 0; the counts add up."""
    cfg = synth.CONFIGS["cfg2"]
    ov = ExactOverlapper(device=0)
    for n, s in synth.oriented(synth.generate_reads(cfg)):
        ov.add_sequence(n, s)
    rows = ov.overlaps_result(1000)
    edges_res, _ = ov.layout_edges(rows)
    rows.free()
    fuzz = 1000
    kept_res, flags = ov.layout_reduce(edges_res, fuzz, want_flags=True)
    st = ov.reduce_stats()
    print("po_reduce_stats at config 2:", st)
    e = edge_array(edges_res.rows())
    kept = edge_array(kept_res.rows())
    kept_res.free()
    edges_res.free()
    ov.close()
    n = len(e)
    assert n > 6_000_000 and st["n_edges_in"] == n and len(flags) == n
    assert set(np.unique(flags).tolist()) <= {0, 1, 2}
    # kept = flag 0, in stage-1 order; counts
    assert np.array_equal(kept, e[flags == 0])
    assert st["n_transitive"] == int((flags == 1).sum()) and st["n_asymmetric"] == int((flags == 2).sum())
    assert st["n_edges_out"] == len(kept) == n - st["n_transitive"] - st["n_asymmetric"]
    assert st["n_transitive"] > n // 2
    # every edge: flag 2 <=> (not transitive itself, and its twin (v^1, u^1) is absent or transitive)
    key = (e[:, 0] << 32) | e[:, 1]
    assert len(np.unique(key)) == n
    srt = np.argsort(key, kind="stable")
    twin = ((e[:, 1] ^ 1) << 32) | (e[:, 0] ^ 1)
    pos = np.minimum(np.searchsorted(key[srt], twin), n - 1)
    present = key[srt][pos] == twin
    twin_gone = ~present | (flags[srt][pos] == 1)
    assert np.array_equal(flags == 2, (flags != 1) & twin_gone)
    # sampled nodes: the rank of an edge is its place in the emission (rows straight from po_overlaps)
    by_src = np.argsort(e[:, 0], kind="stable")
    start = np.searchsorted(e[by_src, 0], np.arange(2 * cfg.n_reads + 1))
    assert st["max_out_degree"] == int(np.diff(start).max())
    rng = np.random.default_rng(2024)
    with_edges = np.flatnonzero(np.diff(start) > 0)
    sample = rng.choice(with_edges, size=2000, replace=False)
    checked = 0
    for v in sample.tolist():
        own = by_src[start[v]:start[v + 1]]
        idx = [own] + [by_src[start[w]:start[w + 1]] for w in e[own, 1].tolist()]
        idx = np.unique(np.concatenate(idx))
        assert len(own) > 0 and np.isin(own, idx).all()                      # the neighbourhood was extracted
        sub = e[idx]
        want = ru.reduce_edges(sub[:, :3], fuzz, rank=idx, nodes=[v])
        mine = sub[:, 0] == v
        assert np.array_equal(want[mine] == 1, flags[idx][mine] == 1), "node %d" % v
        checked += int(mine.sum())
    assert checked > 2000 * 20
