"""The broadcast rules of tests/union_utils.py, proven on the CPU: for every graph stage and both layouts, the stage's CPU
definition run on a union of copies of several cases equals the broadcast of its results on the single cases -- per edge, per
node, tables and counters.  tests/test_gpu_union_scale.py relies on exactly these rules at sizes where the definitions
themselves would be too slow.  Three copies of every case, the cases alternating (A, B, C, A, B, C, ...)."""
import numpy as np
import pytest

import bubblechain_utils as bcu
import components_utils as ccu
import contig_utils as ctu
import partition_utils as ptu
import superbubble_utils as sbu
import union_cases as uc
import union_utils as uu

R = 3


def same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(uu.i64(got[k]), uu.i64(want[k])), (what, k)


def same_stats(got, want, what):
    assert {k: got[k] for k in want} == want, what


@pytest.fixture(scope="module")
def row_singles():
    return [uu.row_pipeline(c[1], c[2]) for c in uc.row_cases()]


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_stages_from_rows(layout, row_singles):
    cases, Ps = uc.row_cases(), row_singles
    U, lengths, rows, seq = uu.row_union(cases, uc.alternating(len(cases), R), layout)
    G = uu.row_pipeline(lengths, rows)                                        # the definitions on the union itself
    W = uu.row_expectation(U, Ps, G["s1"])
    assert G["n_ids"] == U.total_ids and len(rows) == sum(len(c[2]) for c in cases) * R
    # stage 1 and the node order
    s1 = G["s1"]
    assert np.array_equal(s1[np.lexsort((s1[:, 1], s1[:, 0]))], W["s1_sorted"])
    assert np.array_equal(G["order"], W["order"]) and np.array_equal(G["contained"], W["contained"])
    same_stats(G["stage1_stats"], W["stage1_stats"], "stage 1")
    # reduce, tips, diamonds: flags per edge, the node order left, counters
    for stage in ("reduce", "tips", "diamonds"):
        same(G[stage], W[stage], [k for k in ("flags", "left") if k in W[stage]], stage)
        same_stats(G[stage]["stats"], W[stage]["stats"], stage)
        assert G[stage]["flags"].any(), stage + ": the cases give this stage nothing to do"
    # the cleaning chain
    same(G["chain"], W["chain"], ("removed_by", "left"), "chain")
    for got, want in zip(G["chain"]["stats"], W["chain"]["stats"]):
        same_stats(got, want, "chain")
    assert len(set(G["chain"]["removed_by"].tolist())) >= 6
    # merge: flags, renamed edges in input order, node order, the tables in merged%d numbering, counters
    same(G["merge"], W["merge"], ("flags", "edges", "order", "offsets", "members", "prefix", "lengths"), "merge")
    same_stats(G["merge"]["stats"], W["merge"]["stats"], "merge")
    assert G["merge"]["stats"]["n_merged"] >= 3 * R
    heads = G["merge"]["members"][G["merge"]["offsets"][:-1]]
    if layout == "interleaved":                                               # the numbering really alternates between the copies
        assert len(set(U.locate(heads[:6])[0].tolist())) > 1
    # coverage of the stage-1 graph and of the merged graph
    for stage in ("coverage", "coverage_merged"):
        same(G[stage], W[stage], ("read_length_sum", "path_length"), stage)
        same_stats(G[stage]["stats"], W[stage]["stats"], stage)


def graph_check(stage, layout, cases, definition, spec, extra=None):
    """cases: (order, edges[, ...]); definition(case) and definition(union case) must be joined by ``spec``."""
    singles = [definition(c[0], c[1], c) for c in cases]
    width = len(cases[0][1][0])
    U, edges, order, eseq, nseq = uu.graph_union([(c[0], c[1]) for c in cases], uc.alternating(len(cases), R), layout, width)
    got = definition(order.tolist(), [tuple(e) for e in edges.tolist()], None, U, eseq, nseq)
    want = uu.broadcast(U, spec, singles, [c[0] for c in cases], nseq, eseq)
    same(got, want, list(spec["node"]) + list(spec["edge"]) + list(spec["table"]), stage)
    same_stats(got["stats"], want["stats"], stage)
    if extra:
        extra(U, singles, got)
    return got


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_components(layout):
    got = graph_check("components", layout, uc.graph_cases(), lambda order, edges, *_: ccu.weak_components(edges, order), uu.COMPONENTS)
    assert got["stats"]["n_components"] >= R * len(uc.graph_cases())


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_partition(layout):
    got = graph_check("partition", layout, uc.graph_cases(), lambda order, edges, *_: ptu.partition(edges, order), uu.PARTITION)
    assert got["stats"]["n_nonsingleton_sccs"] >= 2 * R


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_superbubbles(layout):
    cases = uc.graph_cases()

    def p_nodes(U, singles, got):
        virtuals = [uu.virtual_nodes(ptu.partition(c[1], c[0])) for c in cases]
        assert got["stats"]["n_p_nodes"] == uu.superbubble_p_nodes(U, singles, virtuals)

    got = graph_check("superbubbles", layout, cases, lambda order, edges, *_: sbu.definition(edges, order), uu.SUPERBUBBLES, p_nodes)
    assert got["stats"]["n_nested"] >= R and got["stats"]["n_discarded"] >= R


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_bubblechains(layout):
    got = graph_check("bubblechains", layout, uc.graph_cases(),
                      lambda order, edges, *_: bcu.definition(edges, order, 1, sbu.definition(edges, order)), uu.BUBBLECHAINS)
    assert got["stats"]["max_chain_bubbles"] >= 2 and got["stats"]["n_chains"] >= 3 * R


@pytest.mark.parametrize("layout", uu.LAYOUTS)
def test_contigs(layout):
    cases = uc.contig_cases()

    def definition(order, edges, case, U=None, eseq=None, nseq=None):
        if case is not None:
            return ctu.definition(edges, order, case[2], case[3], uc.MIN_CONTIG_LEN)
        lengths, exclude = uc.contig_union_inputs(U, cases, nseq)
        return ctu.definition(edges, order, dict(zip(order, lengths.tolist())), [n for n, x in zip(order, exclude.tolist()) if x], uc.MIN_CONTIG_LEN)

    got = graph_check("contigs", layout, cases, definition, uu.CONTIGS)
    st = got["stats"]
    assert st["n_blocked"] >= R and st["n_late_starts"] >= R and st["n_short_paths"] >= R and st["n_isolated"] > st["n_short_isolated"] >= R
