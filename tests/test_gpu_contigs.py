"""The contigs outside the bubble chains on the device (po_layout_contigs, layout.identify_contigs, ``chain-components
--contigs``, ``chain``) against tests/golden/contig_cases.npz: the reference's identify_contigs, unmodified, on the reference's
graphs at two stages and on the direct cases.  Exact integers throughout.  Merged ids reach the device in every stage-(c)
application here."""
import ctypes
import logging

import numpy as np
import pytest

import bubblechain_utils as bu
import components_utils as cu
import contig_utils as ct
import superbubble_utils as su
from phasm_amd import _lib, layout
from phasm_amd.overlapper import ExactOverlapper
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs
from test_contigs_oracle import CASES, check_reference, exclude_of, stage_inputs
from test_gpu_components import FILE_CASES, merge_bytes
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text

pytestmark = pytest.mark.gpu

TEXT_NAMES = ["selfish_1", "tangle_3", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
             [c["name"] for c in CASES if c["name"].startswith("union_")]          # those of tests/test_gpu_bubblechains.py
TEXT = [c for c in CASES if c["name"] in TEXT_NAMES]
assert len(TEXT) == len(TEXT_NAMES) > 6
DIRECT = [c for c in CASES if c.get("direct")]
COUNTS = ct.STAT_KEYS


def as_result(cg):
    none = lambda a: np.where(a == _lib.NO_NODE, ct.NONE, a.astype(np.int64))   # noqa: E731
    t = cg.table
    return {"edge_contig": none(cg.edge_contig), "edge_pos": none(cg.edge_pos), "c_first": t["first_node"].astype(np.int64),
            "c_last": t["last_node"].astype(np.int64), "c_nodes": t["n_nodes"].astype(np.int64), "c_first_edge": none(t["first_edge"]),
            "c_length": t["length"].astype(np.int64), "stats": dict(cg.stats)}


def call_bytes(cg):
    return cg.edge_contig.tobytes() + cg.edge_pos.tobytes() + cg.table.tobytes()


def check_contigs(ov, res, rec, lengths, exclude, golden=True, want_inputs=None):
    """One application on the graph result ``res``: ``exclude`` None (the device's own chains; ``golden``: whether the
    record's X is that set) or the nodes to exclude, passed as bytes; returns the bytes the call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    nodes = order.tolist()
    min_len = rec["min_contig_len"]
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    if exclude is None:
        cg = layout.identify_contigs(ov, res, min_len, 1)
        bc = bu.scheme(e, nodes, 1, su.scheme(e, nodes))
        X = [n for n, c in zip(nodes, bc["node_chain"].tolist()) if c != bu.NONE]
        assert cg.stats["n_chains"] == bc["stats"]["n_chains"]
    else:
        X = list(exclude)
        inside = set(X)
        cg = layout.identify_contigs(ov, res, min_len, 7, np.asarray([n in inside for n in nodes], dtype=np.uint8))   # (min_nodes is ignored)
        assert cg.stats["n_chains"] == 0 and cg.stats["ms_bubblechains"] == 0
    st = cg.stats
    got = as_result(cg)
    if golden:
        ct.check_against_record(got, rec, e)                                             # the golden: the contract's arrays
        check_reference(got, e, rec)                                                     # ... and the reference's paths
        assert {k: st[k] for k in COUNTS} == {k: rec[k] for k in COUNTS}
    want = ct.scheme(e, nodes, lengths, X, min_len)                                      # the restatement, on the device's own edge order
    for k in ct.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: st[k] for k in COUNTS} == {k: want["stats"][k] for k in COUNTS}
    assert cg.edge_contig.dtype == cg.edge_pos.dtype == np.uint32 and cg.table.dtype == _lib.CONTIG_DTYPE
    for j in range(min(len(cg), 20)):
        assert cg.path_of(j) == ct.path_of(want, e, j)
    # the sums that must agree, the rounds within their bounds (both loops read one buffer set and write the other: exactly
    # the rounds of the synchronous scheme), the batches within what the loops allow
    assert st["n_invalid"] == 0 and st["n_nodes"] == len(nodes) and st["n_edges"] == len(e)
    assert st["n_covered_edges"] + st["n_uncovered_edges"] == st["n_edges"]
    assert st["n_contigs"] == st["n_paths"] - st["n_short_paths"] + st["n_isolated"] - st["n_short_isolated"] == len(cg)
    assert int((got["c_nodes"][got["c_first_edge"] != ct.NONE] - 1).sum()) == int((got["edge_contig"] != ct.NONE).sum())
    path_bound, cover_bound = ct.round_bounds(want["stats"])
    assert st["n_path_rounds"] == want["stats"]["n_path_rounds"] <= path_bound
    assert st["n_cover_rounds"] == want["stats"]["n_cover_rounds"] <= cover_bound
    if len(e):
        assert st["n_batches"] >= -(-(st["n_path_rounds"] + st["n_cover_rounds"]) // 8)
    if want_inputs is not None:
        w_edges, w_order = want_inputs[:2]
        assert nodes == list(w_order) and sorted(e[:, :3].tolist()) == sorted(np.asarray(w_edges).reshape(-1, 4)[:, :3].tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s %d %s: %d contigs of %d paths + %d nodes, %d uncovered, rounds %d + %d, %d batches, %.3f ms (chains %.3f, paths %.3f, "
          "cover %.3f, label %.3f)" % (rec["stage"], min_len, "device chains" if exclude is None else "bytes", st["n_contigs"], st["n_paths"],
                                        st["n_isolated"], st["n_uncovered_edges"], st["n_path_rounds"], st["n_cover_rounds"], st["n_batches"],
                                        st["ms_total"], st["ms_bubblechains"], st["ms_paths"], st["ms_cover"], st["ms_label"]))
    return call_bytes(cg)


def check_both(ov, res, case, rec, lengths, want_inputs=None):
    X = exclude_of(case, rec)
    explicit = check_contigs(ov, res, rec, lengths, X, True, want_inputs)
    # a text case's X is the chain set, so the device's own chains give the golden too -- and the same bytes
    own = check_contigs(ov, res, rec, lengths, None, not case.get("direct"), want_inputs)
    if not case.get("direct"):
        assert own == explicit
    return explicit + own


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_contigs_from_gfa_text_equal_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    final = cleaned(ov, edges_res)
    merge_before = merge_bytes(ov, final)
    for rec in case["results"][:2]:
        check_both(ov, final, case, rec, stages["b"][3], stages["b"])            # (b) after the cleaning chain
    assert merge_bytes(ov, final) == merge_before                              # a merge after the calls gives the same bytes
    merged = ov.layout_merge(final)
    for rec in case["results"][2:]:
        check_both(ov, merged, case, rec, stages["c"][3], stages["c"])           # (c) the merged graph: lengths of merged nodes
    assert len(ov) == case["results"][2]["n_ids"]
    for r in (merged, final, edges_res):
        r.free()
    ov.close()


def direct_graph(case, n_ids=None):
    e, order, own_ids, lengths = stage_inputs(case)["a"]
    ov = ExactOverlapper()
    for i in range((n_ids or own_ids) // 2):
        ov.add_segment("s%d" % i, lengths.get(2 * i, 1))
    return ov, ov.graph_from_edges(e, order), (e, order, own_ids, lengths)


@pytest.mark.parametrize("case", DIRECT, ids=[c["name"] for c in DIRECT])
def test_direct_cases_through_graph_from_edges(case):
    ov, g, inputs = direct_graph(case)
    assert len(g) == len(inputs[0]) and g.node_order().tolist() == list(inputs[1])
    check_both(ov, g, case, case["results"][0], inputs[3], inputs)
    g.free()
    ov.close()


def test_three_calls_and_a_fresh_handle_give_identical_bytes(tmp_path):
    case = next(c for c in TEXT if c["name"] == "selfish_1")
    stages = stage_inputs(case)
    seen = []
    for calls in (3, 1):
        ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
        final = cleaned(ov, edges_res)
        merged = ov.layout_merge(final)
        for _ in range(calls):
            seen.append(check_both(ov, final, case, case["results"][1], stages["b"][3]) + check_both(ov, merged, case, case["results"][3], stages["c"][3]))
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    assert len(seen) == 4 and all(s == seen[0] for s in seen)
    for name in ("direct_random_200_seed_3", "direct_comb_300", "direct_path_1025_scrambled"):
        rnd = next(c for c in DIRECT if c["name"] == name)
        seen = []
        for calls in (3, 1):
            ov, g, inputs = direct_graph(rnd)
            seen += [check_both(ov, g, rnd, rnd["results"][0], inputs[3]) for _ in range(calls)]
            g.free()
            ov.close()
        assert all(s == seen[0] for s in seen)


TURN_NAMES = ("direct_two_cycle_entered_from_outside", "direct_path_1025_scrambled", "direct_random_200_seed_1")   # small, large, small


def test_the_five_stages_take_turns_on_one_handle():
    """Components, partition, superbubbles, bubble chains and contigs rank the graph in the same buffers of the handle, and the
    last three run the superbubble stage in the same workspaces: on one handle they alternate on a few nodes, then 1 025, then
    200, so every call finds what a call of another stage -- and, behind the large graph, of a larger graph -- left there.
    Every call's bytes are those of the same call on a handle that has run nothing else."""
    cases = [next(c for c in DIRECT if c["name"] == name) for name in TURN_NAMES]
    inputs = [stage_inputs(c)["a"] for c in cases]
    n_ids = max(i[2] for i in inputs)
    assert [len(i[1]) for i in inputs] == [3, 1025, 200]
    lengths = {}
    for i in inputs[::-1]:
        lengths.update(i[3])                                     # (one handle: one length per segment, the small cases' own win)

    def handle():
        ov = ExactOverlapper()
        for i in range(n_ids // 2):
            ov.add_segment("s%d" % i, lengths.get(2 * i, 1))
        return ov

    def contigs_own(ov, g):
        return ov.layout_contigs(g, 150)

    def contigs_bytes(ov, g):
        return ov.layout_contigs(g, 0, 1, np.arange(len(g.node_order())) % 3 == 0)

    calls = (lambda ov, g: ov.layout_components(g), lambda ov, g: ov.layout_partition(g), lambda ov, g: ov.layout_superbubbles(g),
             lambda ov, g: ov.layout_bubblechains(g), contigs_own, contigs_bytes)

    def fresh(call, e, order):
        ov = handle()
        g = ov.graph_from_edges(e, order)
        out = [a.tobytes() for a in call(ov, g)]
        g.free()
        ov.close()
        return out

    ov = handle()
    for e, order, _, _ in inputs:
        g = ov.graph_from_edges(e, order)
        rows = edge_array(g.rows())
        X = [n for k, n in enumerate(order) if k % 3 == 0]
        want = ct.scheme(rows, list(order), lengths, X, 0)
        got = ov.layout_contigs(g, 0, 1, np.arange(len(order)) % 3 == 0)
        assert np.where(got[0] == _lib.NO_NODE, ct.NONE, got[0].astype(np.int64)).tolist() == want["edge_contig"].tolist()
        assert got[2]["length"].tolist() == want["c_length"].tolist()
        alone = [fresh(call, e, order) for call in calls]
        for k in list(range(len(calls))) + list(range(len(calls)))[::-1] + [2, 4, 3, 5, 4]:
            assert [a.tobytes() for a in calls[k](ov, g)] == alone[k], k
        g.free()
    ov.close()


def test_bubblechain_bytes_and_stats_are_unchanged_by_an_interleaved_contigs_call():
    case = next(c for c in DIRECT if c["name"] == "direct_random_200_seed_2")
    ov, g, _ = direct_graph(case)
    counts = lambda st: {k: v for k, v in st.items() if not k.startswith("ms_")}   # noqa: E731
    first = [a.tobytes() for a in ov.layout_bubblechains(g)]
    stats = counts(ov.bubblechain_stats())
    ov.layout_contigs(g, 0)
    assert counts(ov.bubblechain_stats()) == stats                                    # the other call's stats are its own
    ov.layout_contigs(g, 0, exclude=np.ones(len(g.node_order()), dtype=np.uint8))
    assert [a.tobytes() for a in ov.layout_bubblechains(g)] == first and counts(ov.bubblechain_stats()) == stats
    # exclude = the chain bytes of that call gives the bytes of exclude=None
    chain_bytes = np.frombuffer(first[0], dtype=np.uint32) != _lib.NO_NODE
    assert chain_bytes.any() and not chain_bytes.all()
    assert [a.tobytes() for a in ov.layout_contigs(g, 0, 1, chain_bytes)] == [a.tobytes() for a in ov.layout_contigs(g, 0)]
    g.free()
    ov.close()


def expected_files_and_lines(graph, want, weak):
    """{file name: text} of the contig files of the components, and per component its contigs, from the restatement."""
    order = [int(n) for n in graph.node_order]
    comp_of = dict(zip(order, weak["node_component"].tolist()))
    per = [[] for _ in range(weak["stats"]["n_components"])]
    for c, first in enumerate(want["c_first"].tolist()):
        per[comp_of[first]].append(c)
    files = {}
    for i, contigs in enumerate(per):
        for j, c in enumerate(contigs):
            nodes = list(dict.fromkeys(ct.path_of(want, graph.edges, c)))
            inside = set(nodes)
            edges = np.asarray([x for n in nodes for x in graph.edges.tolist() if x[0] == n and x[1] in inside], dtype=np.int64).reshape(-1, 4)
            files["component%d.contig%d.gfa" % (i, j)] = "".join(layout.component_gfa2_lines(graph, nodes, edges))
    return files, per


@pytest.mark.parametrize("name", FILE_CASES)
def test_the_file_route_with_and_without_the_flag(name, tmp_path, caplog):
    from phasm_amd import cli
    case = next(c for c in CASES if c["name"] == name)
    rec = case["results"][2]                                              # (c), min_contig_len 5000
    text = component_stage_inputs(next(c for c in COMPONENT_CASES if c["name"] == name))["file"]
    p = tmp_path / "graph.gfa"
    p.write_text(text)
    g = layout.chain_components(str(p), bubblechains=True, contigs=True)
    chains_only = layout.chain_components(str(p), bubblechains=True)
    assert chains_only.contigs is None and chains_only.component_contigs is None
    assert chains_only.bubblechains.node_chain.tobytes() == g.bubblechains.node_chain.tobytes()
    # the file numbers its nodes by its own S lines: the stage-(c) graph under other ids than the golden's.  The arrays are
    # the restatement's on the file's own graph; the counts are the golden's, whatever the numbering
    graph = g.graph
    order = [int(n) for n in graph.node_order]
    assert len(order) == rec["n_nodes"] and len(graph.edges) == rec["n_edges"]
    lengths = {n: int(graph.node_length(n)) for n in order}
    bc = bu.scheme(graph.edges, order)
    X = [n for n, c in zip(order, bc["node_chain"].tolist()) if c != bu.NONE]
    want = ct.scheme(graph.edges, order, lengths, X, 5000)
    got = as_result(g.contigs)
    for k in ct.ARRAY_KEYS:
        assert got[k].tolist() == want[k].tolist(), k
    assert {k: g.contigs.stats[k] for k in COUNTS} == {k: rec[k] for k in COUNTS}
    weak = cu.weak_components(graph.edges, order)
    files, per = expected_files_and_lines(graph, want, weak)
    assert g.component_contigs == per
    building = "Building contigs not part of a bubble chain..."
    outs = {}
    for tag, argv in (("plain", ["chain-components"]), ("chains", ["chain-components", "--bubblechains"]),
                      ("contigs", ["chain-components", "--contigs"]), ("both", ["chain-components", "--bubblechains", "--contigs"]),
                      ("chain", ["chain"])):
        out = tmp_path / ("out_" + tag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(argv + [str(p), "-o", str(out), "-f", "gfa2,graphml"]) == 0
        outs[tag] = ({f.name: f.read_text() for f in sorted(out.iterdir())}, [r.getMessage() for r in caplog.records])
    # without the new flag: no contig file, attribute or line (tests/test_gpu_bubblechains.py pins those files against today's)
    for tag in ("plain", "chains"):
        assert not any("contig" in n or "contig" in t for n, t in outs[tag][0].items()) and not any("contig" in m for m in outs[tag][1])
    assert len(outs["plain"][0]) == 2 * len(g.components)
    with_flag, said = outs["contigs"]
    assert outs["both"] == outs["contigs"]                               # --contigs implies --bubblechains
    assert [m for m in said if m != building] == outs["chains"][1] and said.count(building) == len(g.components)
    assert {n: t for n, t in with_flag.items() if "contig" in n and n.endswith(".gfa")} == files
    assert sorted(with_flag) == sorted(list(outs["chains"][0]) + list(files) + [n[:-3] + "graphml" for n in files])
    assert all(with_flag[n] == t for n, t in outs["chains"][0].items() if n.endswith(".gfa") or "bubblechain" in n)
    for i, contigs in enumerate(per):                                    # the edge attribute: j on the edges of the reported paths
        place = {int(x): k for k, x in enumerate(g.components.edges_of(i).tolist())}
        marks = {place[int(x)]: j for j, c in enumerate(contigs) for x in np.flatnonzero(want["edge_contig"] == c).tolist()}
        text_i = with_flag["component%d.graphml" % i]
        assert text_i.count('<data key="d4">') == len(marks)
        plain_i = outs["chains"][0]["component%d.graphml" % i]
        lines = [ln for ln in text_i.splitlines(True) if 'key="d4"' not in ln and 'id="d4"' not in ln]
        assert "".join(lines) == plain_i                                 # nothing else differs from the file without the flag
    # `chain` is `chain-components --bubblechains --contigs` with the reference's last line
    assert outs["chain"][0] == with_flag and outs["chain"][1][:-1] == said[:-1]
    n_chains = sum(len(x) for x in g.component_chains)
    assert outs["chain"][1][-1] == "Built %d bubblechains and %d contigs from %d weakly connected components." % (n_chains, len(g.contigs), len(g.components))
    assert said[-1] == "Wrote %d weakly connected components." % len(g.components)
    # -l drops what it should
    all_lengths = ct.scheme(graph.edges, order, lengths, X, 0)["c_length"]
    if len(all_lengths):
        cut = int(np.sort(all_lengths)[len(all_lengths) // 2]) + 1
        out = tmp_path / "out_l"
        assert cli.main(["chain", str(p), "-o", str(out), "-l", str(cut)]) == 0
        assert sum(1 for f in out.iterdir() if ".contig" in f.name) == int((all_lengths >= cut).sum()) < len(all_lengths)


def test_an_empty_graph_and_null_outputs():
    ov = ExactOverlapper()
    for i in range(4):
        ov.add_segment("s%d" % i, 10 + i)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    for exclude in (None, np.zeros(0, dtype=np.uint8)):
        edge_contig, edge_pos, table = ov.layout_contigs(g, 0, exclude=exclude)
        assert len(edge_contig) == len(edge_pos) == len(table) == 0 and ov.contig_stats()["n_contigs"] == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 4, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    lib = _lib.load()
    excl = np.zeros(4, dtype=np.uint8)
    prm = _lib.PoContigParams(0, 1, 0)
    null = [None, None, None]
    assert lib.po_layout_contigs(ov._h, g._ptr, ctypes.byref(prm), excl.ctypes.data_as(ctypes.c_void_p), *null, ctypes.byref(n)) == _lib.PO_OK
    assert n.value == 2                                                  # the path 0 -> 2 -> 4 and the node 6
    assert lib.po_layout_contigs(ov._h, g._ptr, None, None, *null, ctypes.byref(n)) == _lib.PO_OK and n.value == 0   # 5000 by default
    st = ov.contig_stats()
    assert (st["n_chains"], st["n_excluded"], st["n_blocked"], st["n_isolated"], st["n_short_isolated"]) == (1, 3, 1, 1, 1)
    pos = np.full(2, 7, np.uint32)
    assert lib.po_layout_contigs(ov._h, g._ptr, ctypes.byref(prm), excl.ctypes.data_as(ctypes.c_void_p), None, pos.ctypes.data_as(ctypes.c_void_p),
                                 None, ctypes.byref(n)) == _lib.PO_OK
    assert pos.tolist() == [0, 1]
    table = np.zeros(6, dtype=_lib.CONTIG_DTYPE)
    assert lib.po_layout_contigs(ov._h, g._ptr, ctypes.byref(prm), excl.ctypes.data_as(ctypes.c_void_p), None, None,
                                 table.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)) == _lib.PO_OK
    assert table[:2].tolist() == [(0, 4, 3, 0, 2 + 12), (6, 6, 1, _lib.NO_NODE, 13)]
    g.free()
    ov.close()
