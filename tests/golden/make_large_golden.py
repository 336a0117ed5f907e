#!/usr/bin/env python3
"""Generate tests/golden/large_cases.npz by EXECUTING the reference's own method.

Runs only where the reference checkout is present; the output is committed.

    BubbleChainPhaser.phase_large_bubble  phasm/phasing.py:633-685

run unmodified on an ``object.__new__(BubbleChainPhaser)`` (its constructor wants an assembly graph; the method looks at
``ploidy`` alone), with the reference's own ``OrientedRead``, ``MergedReads``, ``LocalAlignment`` and ``RelevantReadInfo``, on
the paths ``networkx.all_simple_paths`` gives for the case's graph (built edge by edge in edge order, as
``gfa2_reconstruct_assembly_graph`` builds it).  The method returns the winner alone; its ``scored_paths`` dict is read where the
method hands it to ``sorted`` -- through a ``sorted`` in the module's namespace that notes its argument and calls the builtin.

Recorded per case (tests/large_utils.py): graph, node reads, relevant reads, every score, the ``ploidy`` best indices.
Asserted: the paths equal those ``HostPaths`` lists; the scores equal ``large_utils.definition`` bit for bit and the numpy twin
within ``table_tol``; the best list equals both; the margins of ``large_utils.margins_hold``; the walk case's bubble sits between
two ordinary ones."""
import builtins
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")

import networkx  # noqa: E402

import phasm.phasing as ref_phasing  # noqa: E402  (reference)
from phasm.alignments import LocalAlignment, MergedReads, OrientedRead, Read  # noqa: E402  (reference)
from phasm.phasing import BubbleChainPhaser  # noqa: E402  (reference)
from phasm.typing import RelevantReadInfo  # noqa: E402  (reference)

import large_utils as lu  # noqa: E402

assert BubbleChainPhaser.phase_large_bubble.__code__.co_filename.startswith("/root/reference/")

SEEN = []


def noting_sorted(iterable, *args, **kwargs):
    if isinstance(iterable, dict):
        SEEN.append(dict(iterable))
    return builtins.sorted(iterable, *args, **kwargs)


ref_phasing.sorted = noting_sorted


def reference_result(case):
    order, edges = lu.graph_inputs(case)
    reads_of = lu.reads_of_node(case)
    read = {}

    def oriented(r):
        return read.setdefault(int(r), OrientedRead(Read("g%d" % r, 1000), "+"))

    node = {}
    for n in order:
        rs = [int(r) for r in reads_of(n)]
        node[n] = oriented(rs[0]) if rs == [n] or len(rs) == 1 else MergedReads("m%d" % n, 2000, "+", [oriented(r) for r in rs], [500] * (len(rs) - 1))
    g = networkx.DiGraph()
    g.add_nodes_from(node[n] for n in order)
    for u, v, w in edges:
        g.add_edge(node[u], node[v], weight=w)
    hp = lu.host_paths(case)
    b = case["bubble"]
    s, t = int(hp.bubbles["entrance"][b]), int(hp.bubbles["exit"][b])
    paths = [tuple(p) for p in networkx.all_simple_paths(g, node[s], node[t])]
    back = {id(o): n for n, o in node.items()}
    assert [tuple(back[id(x)] for x in p) for p in paths] == hp.paths_of(b), case["name"]
    rel = {}
    for r, om in enumerate(case["overlap_max"]):
        a = OrientedRead(Read("rel%d" % r, 1000), "+")
        lo, hi = case["aln_off"][r], case["aln_off"][r + 1]
        rel[a] = RelevantReadInfo({LocalAlignment(a, oriented(case["b_reads"][x]), (a0, a1), (0, a1 - a0))
                                   for x, a0, a1 in zip(case["aln_b"][lo:hi], case["aln_a0"][lo:hi], case["aln_a1"][lo:hi])}, om)
    ph = object.__new__(BubbleChainPhaser)
    ph.ploidy = case["ploidy"]
    del SEEN[:]
    hs = ph.phase_large_bubble(paths, rel)
    assert len(SEEN) == 1 and len(SEEN[0]) == len(paths)
    scores = [SEEN[0][p] for p in paths]
    index = {p: j for j, p in enumerate(paths)}
    best = [index[p] for p in builtins.sorted(SEEN[0], key=SEEN[0].get, reverse=True)[:case["ploidy"]]]
    assert index[tuple(hs.haplotypes[0])] == best[0] and hs.from_large_bubble
    return {"scores": scores, "best": best}


def main():
    todo = [lu.build(spec) for spec in lu.specs()]
    walk = None
    for seed in range(1, 50):
        walk = lu.walk_inputs(seed)
        case = lu.walk_case(walk)
        if lu.margins_hold(case, lu.definition(case)[0]):
            break
    hp = lu.host_paths(case)
    assert [int(hp.bubbles["n_paths"][b]) for b in hp.chain_bubbles(0)] == [2, 65, 2]
    todo.append(case)
    seen_r, seen_nb, seen_p = set(), set(), set()
    for case in todo:
        ref = reference_result(case)
        scores, best = lu.definition(case)
        assert scores == ref["scores"] and best == ref["best"], case["name"]
        assert lu.margins_hold(case, ref["scores"]), case["name"]
        case["ref"] = ref
        got_best, _, got = lu.twin_scores(case)
        lu.check_scores(got.tolist(), case)
        assert got_best == ref["best"], case["name"]
        seen_r.add(len(case["overlap_max"]))
        seen_nb.add(len(case["b_reads"]))
        seen_p.add(len(scores))
        print("%-22s %4d paths, R %4d, n_b %3d: best %s" % (case["name"], len(scores), len(case["overlap_max"]), len(case["b_reads"]), ref["best"]))
    by = {c["name"]: c for c in todo}
    assert {1, 255, 256, 257, 2048, 2049} <= seen_r and {32, 33, 65} <= seen_nb and {64, 65, 66, 257} <= seen_p
    assert all(s == 0.0 for s in by["all_zero"]["ref"]["scores"]) and by["all_zero"]["ref"]["best"][0] == 0
    tie = by["tie_for_first"]["ref"]
    assert tie["scores"][tie["best"][0]] == tie["scores"][tie["best"][1]] and tie["best"][0] < tie["best"][1]
    assert by["winner_last"]["ref"]["best"][0] == len(by["winner_last"]["ref"]["scores"]) - 1
    assert len(by["p3_n_best_8_r1"]["ref"]["best"]) == 3
    for name in ("p66_bypass_r257", "p66_bypass_first", "permuted"):
        assert 0.0 in by[name]["ref"]["scores"]
    lu.save_golden({"cases": todo})
    print("%d cases, %d bytes" % (len(todo), os.path.getsize(lu.GOLDEN_FILE)))


if __name__ == "__main__":
    main()
