"""Every graph stage on the device at sizes past one capped grid and one scan window, against expectations that cost no
device and no slow walk: unions of disjoint copies of small cases, whose result follows from the CPU definitions on the
single cases by the rules of tests/union_utils.py (proven on the CPU by tests/test_union_rules.py).

A striding kernel runs on at most 8 workgroups of 256 per CU; the one-launch scan handles 262 144 items.  Each union here is
sized so that the stage's own edges, nodes (and for the coverage, rows) exceed 8 * 256 * CUs of the device the test runs on
-- the second trip of every stride loop, the three-kernel scan, sorts over 2**20 keys and a coverage table of millions of
slots all run -- and every test asserts those inequalities, so a test that silently shrank fails.  Both layouts, and one
union of three copies per case (interleaved) per stage: a failure at scale alone is "wrong at scale", a failure of both is
"wrong across copies".

The stages that take rows or a stage-1 result go through GFA2 text and po_add_gfa (35 MB: the threaded reader); the
analysis stages enter through po_graph_from_edges.  Nothing from the device is ever an expectation: the device's stage-1
edge ORDER (a graph has none) only decides in which order the per-edge expectations are laid out."""
import math
import time

import numpy as np
import pytest

import bubblechain_utils as bcu
import components_utils as ccu
import contig_utils as ctu
import diamond_utils as du
import partition_utils as ptu
import superbubble_utils as sbu
import tips_utils as tu
import union_cases as uc
import union_utils as uu
from phasm_amd import _lib, layout
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

UNIONS = [("small", "interleaved"), ("scale", "copy_major"), ("scale", "interleaved")]
IDS = ["%s-%s" % u for u in UNIONS]


def threshold():
    """The threads of one capped grid: what a stage's items must exceed for its stride loops to wrap."""
    import torch
    return 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count


def rounds_for(per_round, size):
    """Copies per case: 3, or as many as bring the smallest per-round count past the threshold."""
    return 3 if size == "small" else -(-(threshold() + 1) // per_round)


def edge_array(e):
    return np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)


def none(a):
    return np.where(a == _lib.NO_NODE, uu.NONE, a.astype(np.int64))


def same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(uu.i64(got[k]), uu.i64(want[k])), (what, k)


def same_stats(st, want, what):
    assert {k: st[k] for k in want} == want, what


def past_threshold(size, **counts):
    """The inequalities of the issue, from result lengths and stats."""
    print("items against the threshold %d: %s" % (threshold(), counts))
    if size == "scale":
        for what, n in counts.items():
            assert n > threshold(), (what, n, threshold())


class Timed:
    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t = time.perf_counter()

    def __exit__(self, *exc):
        print("%s: %.2f s" % (self.what, time.perf_counter() - self.t))


# ---- the stages that start from rows ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def row_singles():
    return [uu.row_pipeline(c[1], c[2]) for c in uc.row_cases()]


class RowUnion:
    pass


@pytest.fixture(scope="module", params=UNIONS, ids=IDS)
def rows_union(request, row_singles, tmp_path_factory):
    """The union as text, read by po_add_gfa, through po_layout_edges; the expectations of every stage laid out along the
    device's stage-1 edges."""
    size, lay = request.param
    cases, Ps = uc.row_cases(), row_singles
    per_round = min(sum(len(c[2]) for c in cases), sum(len(P["s1"]) for P in Ps), sum(len(P["order"]) for P in Ps))
    x = RowUnion()
    x.size, x.layout = size, lay
    x.U, x.lengths, x.rows, seq = uu.row_union(cases, uc.alternating(len(cases), rounds_for(per_round, size)), lay)
    path = tmp_path_factory.mktemp("union") / "union.gfa"
    path.write_text(uu.gfa_text(cases, x.U, seq))
    x.ov = ExactOverlapper()
    n_seg, x.rows_res = x.ov.add_gfa(str(path))
    path.unlink()
    assert n_seg == len(x.lengths)
    got = x.rows_res.rows()
    assert np.array_equal(np.stack([got[k] for k in got.dtype.names], 1).astype(np.int64), x.rows)    # the threaded reader
    x.edges_res, x.removed = x.ov.layout_edges(x.rows_res)
    x.stage1_stats = x.ov.layout_stats()
    x.s1 = edge_array(x.edges_res.rows())
    x.s1_bytes, x.rows_bytes = x.edges_res.rows().tobytes(), x.rows_res.rows().tobytes()
    x.order = x.edges_res.node_order()
    # (the per-edge expectations need every device edge to be an edge of some copy: stage 1 is held to that first)
    srt = x.s1[np.lexsort((x.s1[:, 1], x.s1[:, 0]))]
    want_sorted = uu.stage1_edges(x.U, [P["s1"] for P in Ps])
    x.stage1_ok = np.array_equal(srt, want_sorted)
    x.W = uu.row_expectation(x.U, Ps, x.s1) if x.stage1_ok else None
    yield x
    for r in (x.edges_res, x.rows_res):
        r.free()
    x.ov.close()


def unchanged(x):
    assert x.edges_res.rows().tobytes() == x.s1_bytes and x.rows_res.rows().tobytes() == x.rows_bytes
    assert x.edges_res.node_order().tobytes() == x.order.tobytes()


def test_stage1_edges_and_node_order(rows_union):
    x = rows_union
    assert x.stage1_ok, "po_layout_edges: the edges differ from the copies' stage-1 edges"
    W, st = x.W, x.stage1_stats
    past_threshold(x.size, rows=st["n_rows"], edges=len(x.s1), nodes=len(x.order))
    assert np.array_equal(x.order.astype(np.int64), W["order"])
    assert np.array_equal(x.removed.astype(np.int64), W["contained"])
    same_stats(st, W["stage1_stats"], "stage 1")
    assert st["n_pass"] + st["n_short"] + st["n_min_overlap"] + st["n_overhang"] == st["n_type"][0] + st["n_type"][1]
    with Timed("po_layout_edges again"):
        again, removed = x.ov.layout_edges(x.rows_res)
    assert again.rows().tobytes() == x.s1_bytes and again.node_order().tobytes() == x.order.tobytes() and removed.tobytes() == x.removed.tobytes()
    again.free()
    unchanged(x)


def edge_stage(x, call, stats, want, what, left=True):
    """flags per edge, the kept edges in input order, the node order left, counters; the same bytes twice; inputs untouched."""
    assert x.stage1_ok
    with Timed(what):
        kept, flags = call()
    st = stats()
    assert np.array_equal(flags.astype(np.int64), want["flags"]), what
    assert np.array_equal(edge_array(kept.rows()), x.s1[flags == 0]), what
    assert np.array_equal(kept.node_order().astype(np.int64), want["left"] if left else x.W["order"]), what
    same_stats(st, want["stats"], what)
    kept2, flags2 = call()
    assert flags2.tobytes() == flags.tobytes() and kept2.rows().tobytes() == kept.rows().tobytes()
    assert kept2.node_order().tobytes() == kept.node_order().tobytes()
    kept.free()
    kept2.free()
    unchanged(x)
    return st


def test_reduce(rows_union):
    x = rows_union
    past_threshold(x.size, edges=len(x.s1), nodes=len(x.order))
    edge_stage(x, lambda: x.ov.layout_reduce(x.edges_res, uu.FUZZ, want_flags=True), x.ov.reduce_stats, x.W["reduce"], "po_layout_reduce", left=False)


def test_tips(rows_union):
    x = rows_union
    past_threshold(x.size, edges=len(x.s1), nodes=len(x.order))
    st = edge_stage(x, lambda: x.ov.layout_tips(x.edges_res, uu.TIP_L, uu.TIP_B, want_flags=True), x.ov.tips_stats, x.W["tips"], "po_layout_tips")
    assert st["n_rounds_in"] > 0 and st["n_rounds_out"] > 0
    assert max(st["n_rounds_in"], st["n_rounds_out"]) <= tu.load_golden()["branch_totals"]["max_rounds"]


def test_diamonds(rows_union, row_singles):
    x = rows_union
    past_threshold(x.size, edges=len(x.s1), nodes=len(x.order))
    st = edge_stage(x, lambda: x.ov.layout_diamonds(x.edges_res, want_flags=True), x.ov.diamond_stats, x.W["diamonds"], "po_layout_diamonds")
    # (candidates of different copies share no node: the union needs the rounds of its slowest copy)
    assert 0 < st["n_rounds"] <= max(du.remove_diamond_tips_rounds(P["s1"], P["order"].tolist())[1] for P in row_singles)


def test_cleaning_chain_in_one_call(rows_union):
    x = rows_union
    assert x.stage1_ok
    W = x.W["chain"]
    past_threshold(x.size, edges=len(x.s1), nodes=len(x.order))
    with Timed("clean_assembly_graph"):
        got = layout.clean_assembly_graph(x.ov, x.edges_res, uu.FUZZ, uu.TIP_L, uu.TIP_B)
    assert np.array_equal(got.removed_by.astype(np.int64), W["removed_by"])
    assert np.array_equal(edge_array(got.edges), x.s1[got.removed_by == 0])
    for st, want in zip(got.clean_stats, W["stats"]):
        same_stats(st, want, "chain")
    assert [st["n_edges_in"] for st in got.clean_stats] == [len(x.s1)] + [st["n_edges_out"] for st in got.clean_stats[:3]]
    again = layout.clean_assembly_graph(x.ov, x.edges_res, uu.FUZZ, uu.TIP_L, uu.TIP_B)
    assert again.removed_by.tobytes() == got.removed_by.tobytes() and again.edges.tobytes() == got.edges.tobytes()
    # the node order the chain leaves, from its four calls
    cur = x.edges_res
    for call in (lambda r: x.ov.layout_reduce(r, uu.FUZZ), lambda r: x.ov.layout_tips(r, uu.TIP_L, uu.TIP_B), x.ov.layout_diamonds,
                 lambda r: x.ov.layout_tips(r, uu.TIP_L, tu.DEFAULT_B)):
        nxt = call(cur)
        if cur is not x.edges_res:
            cur.free()
        cur = nxt
    assert np.array_equal(cur.node_order().astype(np.int64), W["left"]) and cur.rows().tobytes() == got.edges.tobytes()
    cur.free()
    unchanged(x)


def merge_arrays(merged):
    offsets, members, prefix, lengths = merged.merged_paths()
    return {"edges": edge_array(merged.rows()), "order": merged.node_order(), "offsets": offsets, "members": members, "prefix": prefix,
            "lengths": lengths}


def test_merge(rows_union):
    x = rows_union
    assert x.stage1_ok
    W = x.W["merge"]
    past_threshold(x.size, edges=len(x.s1), nodes=len(x.order))
    with Timed("po_layout_merge"):
        merged, flags = x.ov.layout_merge(x.edges_res, want_flags=True)
    st = x.ov.merge_stats()
    got = merge_arrays(merged)
    assert np.array_equal(flags.astype(np.int64), W["flags"]) and len(x.ov) == x.U.total_ids
    same(got, W, ("edges", "order", "offsets", "members", "prefix", "lengths"), "merge")     # merged%d numbering: by the heads' ranks
    same_stats(st, W["stats"], "merge")
    assert 0 < st["n_rounds"] <= math.ceil(math.log2(max(st["n_nodes"], 1))) + 1
    merged2, flags2 = x.ov.layout_merge(x.edges_res, want_flags=True)
    got2 = merge_arrays(merged2)
    assert flags2.tobytes() == flags.tobytes() and all(got2[k].tobytes() == got[k].tobytes() for k in got)
    # the coverage of the merged graph: members of merged nodes, lengths of merged nodes
    Wc = x.W["coverage_merged"]
    sums = x.ov.layout_coverage(merged, x.rows_res)
    same(sums, Wc, ("read_length_sum", "path_length"), "coverage of the merged graph")
    same_stats(x.ov.coverage_stats(), Wc["stats"], "coverage of the merged graph")
    merged.free()
    merged2.free()
    unchanged(x)


def test_coverage(rows_union):
    x = rows_union
    assert x.stage1_ok
    W = x.W["coverage"]
    with Timed("po_layout_coverage"):
        sums = x.ov.layout_coverage(x.edges_res, x.rows_res)
    st = x.ov.coverage_stats()
    past_threshold(x.size, rows=st["n_rows"], edges=st["n_edges"], nodes=len(x.order), table_keys=st["n_pairs"])
    same(sums, W, ("read_length_sum", "path_length"), "coverage")
    same_stats(st, W["stats"], "coverage")
    assert st["n_zero_path"] == 0 and st["n_invalid"] == 0
    assert x.ov.layout_coverage(x.edges_res, x.rows_res).tobytes() == sums.tobytes()
    unchanged(x)


# ---- the stages that take any graph: through po_graph_from_edges -----------------------------------------------------------

class GraphUnion:
    pass


def graph_fixture(cases, size, lay, tmp_path_factory):
    g = GraphUnion()
    g.size, g.layout, g.cases = size, lay, cases
    per_round = min(sum(len(c[0]) for c in cases), sum(len(c[1]) for c in cases))
    g.U, g.edges, g.order, g.eseq, g.nseq = uu.graph_union([(c[0], c[1]) for c in cases], uc.alternating(len(cases), rounds_for(per_round, size)), lay)
    g.lengths = uc.segment_lengths(g.U, cases)
    path = tmp_path_factory.mktemp("graph") / "segments.gfa"
    path.write_text(uu.segments_text(g.lengths))
    g.ov = ExactOverlapper()
    n_seg, rows = g.ov.add_gfa(str(path))
    path.unlink()
    rows.free()
    assert 2 * n_seg == g.U.total_ids
    g.res = g.ov.graph_from_edges(g.edges, g.order)
    g.bytes, g.order_bytes = g.res.rows().tobytes(), g.res.node_order().tobytes()
    assert np.array_equal(edge_array(g.res.rows()), g.edges) and np.array_equal(g.res.node_order().astype(np.int64), g.order)
    return g


@pytest.fixture(scope="module", params=UNIONS, ids=IDS)
def graph_union(request, tmp_path_factory):
    g = graph_fixture(uc.graph_cases(), *request.param, tmp_path_factory)
    yield g
    g.res.free()
    g.ov.close()


@pytest.fixture(scope="module", params=UNIONS, ids=IDS)
def contig_union(request, tmp_path_factory):
    g = graph_fixture(uc.contig_cases(), *request.param, tmp_path_factory)
    yield g
    g.res.free()
    g.ov.close()


def graph_stage(g, what, call, as_result, single, spec):
    """One analysis call on the union against the broadcast of ``single`` on every case; the same bytes twice; inputs untouched."""
    past_threshold(g.size, edges=len(g.edges), nodes=len(g.order))
    singles = [single(c) for c in g.cases]
    want = uu.broadcast(g.U, spec, singles, [c[0] for c in g.cases], g.nseq, g.eseq)
    with Timed(what):
        out = call()
    got = as_result(out)
    same(got, want, list(spec["node"]) + list(spec["edge"]) + list(spec["table"]), what)
    same_stats(got["stats"], want["stats"], what)
    assert got["stats"]["n_invalid"] == 0
    assert [a.tobytes() for a in call()] == [a.tobytes() for a in out]
    assert g.res.rows().tobytes() == g.bytes and g.res.node_order().tobytes() == g.order_bytes
    return got["stats"], singles


def test_components(graph_union):
    g = graph_union
    st, _ = graph_stage(g, "po_layout_components", lambda: g.ov.layout_components(g.res, len(g.order)),
                        lambda o: {"node_component": o[0], "edge_component": o[1], "stats": g.ov.components_stats(),
                                   **{k: o[2][k] for k in ("first_node", "n_nodes", "n_edges")}},
                        lambda c: ccu.weak_components(c[1], c[0]), uu.COMPONENTS)
    assert 0 < st["n_rounds"] <= len(g.order) + 2


def test_partition(graph_union):
    g = graph_union
    st, _ = graph_stage(g, "po_layout_partition", lambda: g.ov.layout_partition(g.res, len(g.order)),
                        lambda o: {"node_scc": o[0], "node_flags": o[1], "edge_class": o[2], "stats": g.ov.partition_stats(),
                                   **{k: o[3][k] for k in ("first_node", "n_nodes", "n_edges", "n_r_in", "n_re_out")}},
                        lambda c: ptu.partition(c[1], c[0]), uu.PARTITION)
    n = len(g.order)
    assert sum(st["n_class"]) == st["n_edges"] and 0 < st["n_outer"] <= n
    assert all(st[k] <= st["n_outer"] * (n + 2) for k in ("n_trim_rounds", "n_forward_rounds", "n_backward_rounds"))


def test_superbubbles(graph_union):
    g = graph_union
    st, singles = graph_stage(g, "po_layout_superbubbles", lambda: g.ov.layout_superbubbles(g.res, len(g.order)),
                              lambda o: {"node_exit": none(o[0]), "node_inside": none(o[1]), "node_flags": o[2], "stats": g.ov.superbubble_stats(),
                                         "b_entrance": o[3]["entrance"], "b_exit": o[3]["exit"], "b_inside": o[3]["n_inside"],
                                         "b_nested": o[3]["nested"]},
                              lambda c: sbu.definition(c[1], c[0]), uu.SUPERBUBBLES)
    virtuals = [uu.virtual_nodes(ptu.partition(c[1], c[0])) for c in g.cases]
    assert st["n_p_nodes"] == uu.superbubble_p_nodes(g.U, singles, virtuals)
    schemes = [sbu.scheme(c[1], c[0])["stats"] for c in g.cases]
    # (levels are longest paths: the union has those of its deepest copy; rounds only within their caps)
    assert (st["n_levels_forward"], st["n_levels_backward"]) == tuple(max(s[k] for s in schemes) for k in ("n_levels_forward", "n_levels_backward"))
    assert 1 <= st["n_level_rounds"] <= max(st["n_levels_forward"], st["n_levels_backward"], 1) + 1
    assert 0 < st["n_discard_rounds"] <= max(s["n_discard_rounds"] for s in schemes)


def test_bubblechains(graph_union):
    g = graph_union
    st, _ = graph_stage(g, "po_layout_bubblechains", lambda: g.ov.layout_bubblechains(g.res, 1, len(g.order)),
                        lambda o: {"node_chain": none(o[0]), "node_bubble": none(o[1]), "edge_chain": none(o[2]), "stats": g.ov.bubblechain_stats(),
                                   "c_first": o[3]["first_entrance"], "c_last": o[3]["last_exit"], "c_bubbles": o[3]["n_bubbles"],
                                   "c_nodes": o[3]["n_nodes"], "c_edges": o[3]["n_edges"]},
                        lambda c: bcu.definition(c[1], c[0], 1, sbu.definition(c[1], c[0])), uu.BUBBLECHAINS)
    levels = max(sbu.scheme(c[1], c[0])["stats"]["n_levels_forward"] for c in g.cases)
    nest_bound, chain_bound = bcu.round_bounds({"n_levels_forward": levels, "max_chain_bubbles": st["max_chain_bubbles"]})
    assert 0 < st["n_nest_rounds"] <= nest_bound and 0 < st["n_chain_rounds"] <= chain_bound


def contig_result(g):
    return lambda o: {"edge_contig": none(o[0]), "edge_pos": none(o[1]), "stats": g.ov.contig_stats(), "c_first": o[2]["first_node"],
                      "c_last": o[2]["last_node"], "c_nodes": o[2]["n_nodes"], "c_first_edge": none(o[2]["first_edge"]), "c_length": o[2]["length"]}


def contig_rounds(st, schemes):
    path_bound, cover_bound = ctu.round_bounds({k: max(s[k] for s in schemes) for k in ("max_path_depth", "max_cover_depth")})
    assert 0 < st["n_path_rounds"] <= path_bound and 0 < st["n_cover_rounds"] <= cover_bound
    assert st["n_covered_edges"] + st["n_uncovered_edges"] == st["n_edges"]


def test_contigs_with_given_exclusions(contig_union):
    g = contig_union
    _, exclude = uc.contig_union_inputs(g.U, g.cases, g.nseq)
    st, _ = graph_stage(g, "po_layout_contigs", lambda: g.ov.layout_contigs(g.res, uc.MIN_CONTIG_LEN, 7, exclude, len(g.order)), contig_result(g),
                        lambda c: ctu.definition(c[1], c[0], c[2], c[3], uc.MIN_CONTIG_LEN), uu.CONTIGS)
    contig_rounds(st, [ctu.scheme(c[1], c[0], c[2], c[3], uc.MIN_CONTIG_LEN)["stats"] for c in g.cases])
    assert st["n_chains"] == 0


def test_contigs_outside_the_device_s_own_chains(graph_union):
    g = graph_union

    def inputs(c):
        order, edges = c
        chains = bcu.definition(edges, order, 1, sbu.definition(edges, order))
        return edges, order, {n: 1000 for n in order}, [n for n, j in zip(order, chains["node_chain"].tolist()) if j != bcu.NONE], 1500

    st, _ = graph_stage(g, "po_layout_contigs (own chains)", lambda: g.ov.layout_contigs(g.res, 1500, 1, None, len(g.order)), contig_result(g),
                        lambda c: ctu.definition(*inputs(c)), uu.CONTIGS)
    contig_rounds(st, [ctu.scheme(*inputs(c))["stats"] for c in g.cases])
    assert st["n_chains"] > 0 and st["n_short_paths"] > 0
