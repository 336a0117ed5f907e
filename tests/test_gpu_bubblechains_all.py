"""The bubble chains and the contigs of the whole graph on the device, ring chains included (po_layout_bubblechains_all,
po_layout_contigs_all, ``layout.bubble_chains(..., cyclic=True)``, ``layout.identify_contigs(..., cyclic=True)``,
``chain --cyclic``) against tests/golden/bubblechain_all_cases.npz: the ring-aware restatement of the reference's walk, held
equal to the scheme and held against the reference's own build_bubblechains and identify_contigs by
tests/golden/make_bubblechains_all_golden.py.  Exact integers throughout.  The one direct case with merged-node ids cannot
go through po_graph_from_edges; merged ids reach the device in every stage-(c) application here."""
import ctypes
import logging
import time

import numpy as np
import pytest

import bubblechain_all_utils as ba
import bubblechain_utils as bu
import components_utils as cu
import contig_utils as ct
import cyclic_utils as cy
import union_cases as uc
import union_utils as uu
from phasm_amd import _lib, layout
from phasm_amd.overlapper import ExactOverlapper
from test_bubblechains_all_oracle import CASES, check_input, contig_check, exclude_of, stage_inputs
from test_bubblechains_files import graph_text
from test_gpu_components import segments
from test_gpu_merge import BY_NAME as MERGE_BY_NAME, cleaned, edge_array, edges_from_text

pytestmark = pytest.mark.gpu

TEXT = [c for c in CASES if not c.get("direct")]
DIRECT = [c for c in CASES if c.get("direct") and not c.get("host_only")]
assert len(DIRECT) == sum(1 for c in CASES if c.get("direct")) - 1
RESTATE_UP_TO = 3000          # nodes: above, the golden's digest alone holds the arrays (the restatement takes seconds there)


def none(a):
    return np.where(a == _lib.NO_NODE, ba.NONE, a.astype(np.int64))


def as_result(bc):
    return ba.as_result(bc.stats, (bc.node_chain, bc.node_bubble, bc.edge_chain, bc.table))


def contig_result(cg):
    t = cg.table
    return {"edge_contig": none(cg.edge_contig), "edge_pos": none(cg.edge_pos), "c_first": t["first_node"].astype(np.int64),
            "c_last": t["last_node"].astype(np.int64), "c_nodes": t["n_nodes"].astype(np.int64), "c_first_edge": none(t["first_edge"]),
            "c_length": t["length"].astype(np.int64), "stats": dict(cg.stats)}


def call_bytes(bc):
    return bc.node_chain.tobytes() + bc.node_bubble.tobytes() + bc.edge_chain.tobytes() + bc.table.tobytes()


def check_all(ov, res, rec, lengths=None, want_inputs=None):
    """One application on the graph result ``res`` against its record: the chains, then the contigs outside them with X built
    on the device and with X passed in.  Returns the bytes the chain call gave back."""
    before, order = res.rows().tobytes(), res.node_order()
    min_nodes, nodes = rec["min_nodes"], order.tolist()
    bc = layout.bubble_chains(ov, res, min_nodes, cyclic=True)
    st = bc.stats
    e = edge_array(res.rows()) if len(res) else np.zeros((0, 4), np.int64)
    got = as_result(bc)
    ba.check_against_record(got, rec, e)                                                 # the golden: arrays, table, stats
    assert {k: st[k] for k in ba.SCHEME_KEYS} == {k: rec[k] for k in ba.SCHEME_KEYS}
    assert bc.node_chain.dtype == bc.node_bubble.dtype == bc.edge_chain.dtype == np.uint32 and bc.table.dtype == _lib.BUBBLECHAIN_DTYPE
    n = len(nodes)
    assert st["n_invalid"] == 0 and st["n_nodes"] == n and st["n_edges"] == len(e)
    assert st["n_ring_rounds"] == (ba.ring_rounds(st["n_top"]) if st["n_top"] and st["n_cyclic_bubbles"] else 0)
    if n:
        assert (st["n_chain_rounds"] > 0) == (st["n_top"] > 0) and st["n_chain_rounds"] <= bu.log2_ceil(max(st["max_chain_bubbles"], 2)) + 2
    if n <= RESTATE_UP_TO:
        want = ba.scheme(e, nodes, min_nodes)                                            # the restatement, on the device's own edge order
        for k in ba.ARRAY_KEYS:
            assert got[k].tolist() == want[k].tolist(), k
        for j in range(min(len(bc), 20)):
            assert bc.nodes_of(j).tolist() == bu.nodes_of(want, nodes, j) and len(bc.edges_of(j)) == want["c_edges"][j]
            walk = bc.bubbles_of(j)
            assert len(walk) == want["c_bubbles"][j] and walk[-1][1] == want["c_last"][j] and len({s for s, _ in walk}) == len(walk)
    # no non-singleton SCC: byte-equal to po_layout_bubblechains
    ov.layout_partition(res, n)
    if ov.partition_stats()["n_nonsingleton_sccs"] == 0:
        old = layout.bubble_chains(ov, res, min_nodes)
        assert call_bytes(old) == call_bytes(bc) and st["n_ring_chains"] == 0
        assert {k: old.stats[k] for k in bu.STAT_KEYS} == {k: st[k] for k in bu.STAT_KEYS}
    # the contigs: X built on the device (both minimum lengths), X passed in (the first)
    X = exclude_of(got, nodes)
    flags = np.isin(order, np.asarray(X, dtype=order.dtype)).astype(np.uint8)
    for k, crec in enumerate(rec["contigs"]):
        own = layout.identify_contigs(ov, res, crec["min_contig_len"], min_nodes, cyclic=True)
        c_got = contig_result(own)
        contig_check(c_got, crec, e)
        assert own.stats["n_chains"] == st["n_chains"] and own.stats["n_excluded"] == len(X)
        if lengths is not None and n <= RESTATE_UP_TO:
            c_want = ct.scheme(e, nodes, lengths, X, crec["min_contig_len"])
            for key in ct.ARRAY_KEYS:
                assert c_got[key].tolist() == c_want[key].tolist(), key
        if k == 0:
            given = layout.identify_contigs(ov, res, crec["min_contig_len"], min_nodes, exclude=flags, cyclic=True)
            assert [given.edge_contig.tobytes(), given.edge_pos.tobytes(), given.table.tobytes()] == \
                [own.edge_contig.tobytes(), own.edge_pos.tobytes(), own.table.tobytes()] and given.stats["n_chains"] == 0
    if want_inputs is not None:
        w_edges, w_order = want_inputs[0], want_inputs[1]
        assert nodes == list(w_order) and sorted(e[:, :2].tolist()) == sorted(cu.uv_of(w_edges).tolist())
    assert res.rows().tobytes() == before and res.node_order().tobytes() == order.tobytes()     # the inputs stay as they were
    print("%s: %d chains (%d short), %d rings of %d bubbles, election %d rounds, ranking %d, %d batches, %.3f ms (superbubbles %.3f, chains %.3f, "
          "label %.3f)" % (rec["stage"], st["n_chains"], st["n_short"], st["n_ring_chains"], st["n_ring_bubbles"], st["n_ring_rounds"],
                           st["n_chain_rounds"], st["n_batches"], st["ms_total"], st["ms_superbubbles"], st["ms_chains"], st["ms_label"]))
    return call_bytes(bc)


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_from_gfa_text_equals_the_golden(case, tmp_path):
    stages = stage_inputs(case)
    ov, edges_res = edges_from_text(MERGE_BY_NAME[case["name"]], tmp_path)
    rec_b, rec_c = case["results"]
    final = cleaned(ov, edges_res)
    check_all(ov, final, rec_b, stages["b"][3], stages["b"])               # (b) after the cleaning chain
    merged = ov.layout_merge(final)
    check_all(ov, merged, rec_c, stages["c"][3], stages["c"])              # (c) the merged graph: node ids >= the reads
    for r in (merged, final, edges_res):
        r.free()
    ov.close()


def direct_graph(case):
    e4, order, n_ids, lengths = stage_inputs(case)["a"]
    ov = segments(n_ids)
    return ov, ov.graph_from_edges(e4, order), (e4, order, n_ids, lengths)


@pytest.mark.parametrize("case", DIRECT, ids=[c["name"] for c in DIRECT])
def test_direct_cases_through_graph_from_edges(case):
    ov, g, inputs = direct_graph(case)
    assert len(g) == len(inputs[0]) and g.node_order().tolist() == list(inputs[1])
    check_input(inputs[0], inputs[1], inputs[3], case["results"][0])
    check_all(ov, g, case["results"][0], inputs[3], inputs)
    g.free()
    ov.close()


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("direct_rc_ring_of_16_bubbles_scrambled", "direct_rc_ring_beside_a_path_chain", "direct_cy_ring_of_16_diamonds_interior_lowest",
                 "direct_ring_1025_scrambled", "direct_random_200_500_seed2"):
        case = next(c for c in DIRECT if c["name"] == name)
        seen = []
        for calls in (2, 1):
            ov, g, _ = direct_graph(case)
            seen += [check_all(ov, g, case["results"][0]) for _ in range(calls)]
            g.free()
            ov.close()
        assert len(seen) == 3 and all(s == seen[0] for s in seen), name


def test_the_calls_take_turns_with_their_siblings_on_one_handle():
    """The calls work in the workspaces of po_layout_superbubbles_all and po_layout_bubblechains: behind them, and behind a
    larger graph, the siblings and the calls themselves still give the bytes of a fresh handle."""
    names = ("direct_rc_ring_of_5_bubbles_scrambled", "direct_ring_1025_scrambled", "direct_rc_ring_with_a_nested_bubble")   # small, large, small
    inputs = [stage_inputs(next(c for c in DIRECT if c["name"] == n))["a"] for n in names]
    n_ids = max(i[2] for i in inputs)
    calls = (lambda ov, g: ov.layout_superbubbles_all(g), lambda ov, g: ov.layout_bubblechains(g), lambda ov, g: ov.layout_bubblechains_all(g),
             lambda ov, g: ov.layout_contigs(g, 0), lambda ov, g: ov.layout_contigs_all(g, 0), lambda ov, g: ov.layout_superbubbles(g))

    def fresh(call, e4, order):
        ov = segments(n_ids)
        g = ov.graph_from_edges(e4, order)
        out = b"".join(a.tobytes() for a in call(ov, g))
        g.free()
        ov.close()
        return out

    ov = segments(n_ids)
    for e4, order, _, _ in inputs:
        g = ov.graph_from_edges(e4, order)
        alone = [fresh(call, e4, order) for call in calls]
        for k in (0, 1, 2, 3, 4, 5, 4, 2, 3, 1, 2, 0, 2):
            assert b"".join(a.tobytes() for a in calls[k](ov, g)) == alone[k], k
        g.free()
    ov.close()


def test_an_empty_graph_and_null_outputs():
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), np.int64), [])
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains_all(g)
    assert len(node_chain) == len(node_bubble) == len(edge_chain) == len(table) == 0 and ov.bubblechain_all_stats()["n_chains"] == 0
    assert len(ov.layout_contigs_all(g, 0)[2]) == 0
    g.free()
    g = ov.graph_from_edges(np.asarray([[0, 2, 1, 1], [2, 4, 1, 1], [4, 0, 1, 1], [6, 6, 1, 1]]), [0, 2, 4, 6])
    n = ctypes.c_uint64(99)
    lib = _lib.load()
    assert lib.po_layout_bubblechains_all(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 1
    st = ov.bubblechain_all_stats()
    assert (st["n_chains"], st["n_ring_chains"], st["n_ring_bubbles"], st["n_cyclic_bubbles"], st["n_root_runs"]) == (1, 1, 3, 3, 1)
    table = np.zeros(4, _lib.BUBBLECHAIN_DTYPE)
    assert lib.po_layout_bubblechains_all(ov._h, g._ptr, None, None, None, None, table.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.byref(n)) == _lib.PO_OK
    assert table[:1].tolist() == [(0, 0, 3, 3, 3)]
    assert lib.po_layout_contigs_all(ov._h, g._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_OK and n.value == 0
    assert ov.contig_stats()["n_excluded"] == 3 and ov.contig_stats()["n_chains"] == 1
    g.free()
    ov.close()


def test_the_chain_command_on_a_ring_file(tmp_path, caplog):
    """`chain --cyclic` on a file whose one component is a ring of three diamonds: one chain file that holds every node and no
    contig cut out of it; without the flag, today's answer: no chain, and pieces of the ring as contigs."""
    from phasm_amd import cli
    D = cy._diamond
    ring = [e for i in range(3) for e in D(6 * i, 6 * i + 2, 6 * i + 4, 6 * ((i + 1) % 3))]
    p = tmp_path / "ring.gfa"
    p.write_text(graph_text(9, ring))
    outs = {}
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=cli.logger.name):
            assert cli.main(["chain", str(p), "-o", str(out), "-l", "0"] + (["--cyclic"] if flag else [])) == 0
        outs[flag] = (sorted(f.name for f in out.iterdir()), [r.getMessage() for r in caplog.records][-1])
    assert outs[True] == (["component0.bubblechain0.gfa", "component0.gfa"], "Built 1 bubblechains and 0 contigs from 1 weakly connected components.")
    assert (tmp_path / "out1" / "component0.bubblechain0.gfa").read_text() == (tmp_path / "out1" / "component0.gfa").read_text()
    assert "component0.bubblechain0.gfa" not in outs[False][0] and outs[False][1].startswith("Built 0 bubblechains")
    g = layout.chain_components(str(p), bubblechains=True, contigs=True, min_length=0, cyclic=True)
    assert g.bubblechains.bubbles_of(0) == [(0, 6), (6, 12), (12, 0)] and len(g.contigs) == 0
    assert g.bubblechains.nodes_of(0).tolist() == g.components.nodes_of(0).tolist() and g.bubblechains.stats["n_ring_chains"] == 1


# ---- one union past a capped grid ---------------------------------------------------------------------------------------

def threshold():
    """The threads of one capped grid: what the ranks must exceed for the stride loops to wrap."""
    import torch
    return 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count


SPEC = dict(uu.BUBBLECHAINS, add=uu.BUBBLECHAINS["add"] + ("n_ring_chains", "n_ring_bubbles", "n_cyclic_bubbles"))


@pytest.mark.parametrize("lay", uu.LAYOUTS)
def test_a_union_of_rings_and_path_chains_past_one_grid(lay, tmp_path):
    """Copies of the 6-node ring, of ring_of_3_diamonds and of a small path chain, just over one capped grid of ranks (524 288
    on 256 CUs), in both layouts; the expectation is broadcast from the three single results by the rules of union_utils."""
    D = cy._diamond
    o2, e2 = cy.ring_of_diamonds(2)
    o3, e3 = cy.ring_of_diamonds(3)
    cases = [(o2, e2), (o3, e3), ([2 * i for i in range(7)], D(0, 2, 4, 6) + D(6, 8, 10, 12))]
    cases = [(o, [(u, v, 100, 17) for u, v in e]) for o, e in cases]
    per_round = sum(len(o) for o, _ in cases)
    copies = uc.alternating(len(cases), -(-(threshold() + 1) // per_round))
    U, edges, order, eseq, nseq = uu.graph_union(cases, copies, lay)
    assert len(order) > threshold() and len(order) - threshold() <= per_round
    singles = [ba.scheme(np.asarray(e, np.int64), o, 1) for o, e in cases]
    assert [s["stats"]["n_ring_chains"] for s in singles] == [1, 1, 0]
    want = uu.broadcast(U, SPEC, singles, [o for o, _ in cases], nseq, eseq)
    path = tmp_path / "segments.gfa"
    path.write_text(uu.segments_text(np.full(U.total_ids // 2, 1000, np.int64)))
    ov = ExactOverlapper()
    n_seg, rows = ov.add_gfa(str(path))
    rows.free()
    assert 2 * n_seg == U.total_ids
    res = ov.graph_from_edges(edges, order)
    before = res.rows().tobytes()
    t0 = time.perf_counter()
    out = ov.layout_bubblechains_all(res, 1, len(order))
    print("po_layout_bubblechains_all on %d ranks (%s): %.2f s" % (len(order), lay, time.perf_counter() - t0))
    st = ov.bubblechain_all_stats()
    got = ba.as_result(st, out)
    for k in list(SPEC["node"]) + list(SPEC["edge"]) + list(SPEC["table"]):
        assert np.array_equal(uu.i64(got[k]), uu.i64(want[k])), k
    assert {k: st[k] for k in want["stats"]} == want["stats"]
    assert st["n_ring_chains"] == 2 * (len(copies) // 3) and st["n_ring_rounds"] == ba.ring_rounds(st["n_top"]) and st["n_invalid"] == 0
    assert [a.tobytes() for a in ov.layout_bubblechains_all(res, 1, len(order))] == [a.tobytes() for a in out]
    assert res.rows().tobytes() == before
    res.free()
    ov.close()
