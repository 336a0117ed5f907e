#!/usr/bin/env python3
"""Generate tests/golden/relevant_cases.npz by EXECUTING the reference's own methods.

Runs only where the reference checkout is present; the output (inputs and recorded results only) is committed.

    BubbleChainPhaser.get_aligning_reads          phasm/phasing.py:541-550
    BubbleChainPhaser.get_relevant_read_info      phasm/phasing.py:366-404
    BubbleChainPhaser._get_max_possible_overlap   phasm/phasing.py:406-419
    BubbleChainPhaser.new_block                   phasm/phasing.py:343-364   (the fallback cases: new_block(), then the call)

run unmodified on an ``object.__new__(BubbleChainPhaser)`` whose attributes are set by hand, as make_phase_golden.py does.
``self.g`` is a stub with ``predecessors_iter``, ``__getitem__`` and ``edge_len`` (networkx here is 3.4: the real graph class has
no ``predecessors_iter``); among the predecessors of every exit it holds one ``MergedReads`` node, which is never a key of the
mapping and must yield ``len(read)``.

``alignments`` is built from GFA2 ``E`` lines by the reference's ``gfa2_line_to_la`` and ``LocalAlignment.switch`` in the loop of
``_get_read_alignments`` (phasm/cli/assembler.py:313-328), restated below line for line: that module itself does not import
here, because dinopy is absent.  The two set expressions of ``phase()`` between the calls (phasing.py:263-264, 283-284) are
restated as well; ``phase()`` itself walks a graph.

Recorded per case: the index (offsets and entries in ascending (x, y), from ``definition`` -- the sequence numbers are not a
thing the reference keeps) after the reference's mapping was found equal to it entry for entry; per query the RESULT of
tests/relevant_utils.py, every field that the reference computes taken from the reference, ``b_reads`` from ``definition``.
Beside the cases: the time of the reference's dict build and of ``get_relevant_read_info`` on a host core."""
import os
import sys
import time
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")

from phasm.alignments import MergedReads, Read  # noqa: E402  (reference)
from phasm.io import gfa  # noqa: E402  (reference)
from phasm.phasing import BubbleChainPhaser, HaplotypeSet  # noqa: E402  (reference)

import relevant_utils as ru  # noqa: E402
from phasm_amd import phasing  # noqa: E402

assert BubbleChainPhaser.get_relevant_read_info.__code__.co_filename.startswith("/root/reference/")


def oriented_name(x):
    return "s%d%s" % (x // 2, "+-"[x & 1])


def e_lines(case):
    for a, b, astart, aend, bstart, bend in ru.rows_of(case).tolist():
        yield "E\t*\t%s\t%s\t%d\t%d\t%d\t%d\t*\n" % (oriented_name(a), oriented_name(b), astart, aend, bstart, bend)


def read_alignments(lines, reads):
    """The loop of ``_get_read_alignments`` (assembler.py:316-328)."""
    read_alignments = defaultdict(dict)
    la_iter = map(gfa.gfa2_line_to_la(reads), (l for l in lines if l.startswith('E')))
    for la in la_iter:
        a_read, b_read = la.get_oriented_reads()
        read_alignments[a_read][b_read] = la
        read_alignments[b_read][a_read] = la.switch()
    return read_alignments


class StubGraph:
    """What ``get_relevant_read_info`` asks of the assembly graph."""
    edge_len = "weight"

    def __init__(self, exit_node, preds):
        self.exit_node = exit_node
        self.preds = preds                      # node -> edge_len

    def predecessors_iter(self, node):
        assert node is self.exit_node
        return iter(self.preds)

    def __getitem__(self, pred):
        return {self.exit_node: {self.edge_len: self.preds[pred]}}


def reference_result(case, q, alignments, oriented, ident):
    ph = object.__new__(BubbleChainPhaser)
    ph.alignments = alignments
    ph.ploidy = 2
    ph.min_spanning_reads = q["min_span"]
    ph.start_of_block = q["mode"] == 1
    ph.prev_graph_reads = {oriented[x] for x in q["prev_graph"]}
    ph.prev_aligning_reads = {oriented[x] for x in q["prev_aligning"]}
    ph.candidate_sets = [HaplotypeSet(2)]
    exit_node = Read("exit", 300).with_orientation("+")
    preds = {oriented[p]: e for p, e in q["preds"]}
    merged = MergedReads("merged", 500, "+", [oriented[0], oriented[1]], [7])
    preds[merged] = 1                           # edge_len - sum(prefix_lengths) = -6: it would win every minimum if it counted
    ph.g = StubGraph(exit_node, preds)
    cur_bubble_graph_reads = {oriented[x] for x in q["cur_graph"]}
    out = {k: [] for k in ru.RESULT_KEYS}
    out.update(n_spanning=0, fell_back=0, aln_off=[0])
    if not cur_bubble_graph_reads:
        return out
    cur_bubble_aligning_reads = ph.get_aligning_reads(list(cur_bubble_graph_reads))
    spanning_reads = (ph.prev_aligning_reads & cur_bubble_aligning_reads)                    # phasing.py:263-264
    if (len(spanning_reads) < ph.min_spanning_reads and not ph.start_of_block):              # phasing.py:266-267
        ph.new_block()
        out["fell_back"] = 1
    relevant_reads = (spanning_reads if not ph.start_of_block else cur_bubble_aligning_reads)   # phasing.py:283-284
    info = ph.get_relevant_read_info(relevant_reads, cur_bubble_graph_reads, exit_node)
    assert set(info) == set(relevant_reads)
    out["cur_aligning"] = sorted(ident[r] for r in cur_bubble_aligning_reads)
    out["n_spanning"] = len(spanning_reads)
    out["rel_reads"] = sorted(ident[r] for r in info)
    by_id = {ident[r]: v for r, v in info.items()}
    for r in out["rel_reads"]:
        las, om = by_id[r]
        for y, a0, a1 in sorted((ident[la.get_oriented_reads()[1]], la.arange[0], la.arange[1]) for la in las):
            out["aln_y"].append(y)
            out["aln_a0"].append(a0)
            out["aln_a1"].append(a1)
        out["aln_off"].append(len(out["aln_y"]))
        out["overlap_max"].append(om)
    return out, info


def main():
    cases, timings = [], {}
    for name, spec in ru.SPECS.items():
        case = spec()
        reads = {"s%d" % i: Read("s%d" % i, n) for i, n in enumerate(case["lengths"])}
        oriented = [reads["s%d" % (x // 2)].with_orientation("+-"[x & 1]) for x in range(2 * case["n_seg"])]
        ident = {r: x for x, r in enumerate(oriented)}
        lines = list(e_lines(case))
        t0 = time.perf_counter()
        alignments = read_alignments(lines, reads)
        timings[name + ".dict_build_ms"] = (time.perf_counter() - t0) * 1e3
        # the reference's mapping, entry for entry, against the definition
        m = ru.mapping(case)
        assert {ident[a] for a in alignments} == set(m)
        for a, d in alignments.items():
            assert {ident[b]: la.arange for b, la in d.items()} == {y: v[:2] for y, v in m[ident[a]].items()}, name
            assert all(la.get_oriented_reads() == (a, b) for b, la in d.items())
        off, entries = ru.index_definition(case)
        case["index_off"] = off
        case["index_b"], case["index_a0"], case["index_a1"], case["index_seq"] = (list(v) for v in zip(*entries))
        host = phasing.HostIndex(ru.lengths_of(case))
        hidx = host.phase_index(ru.rows_of(case))
        ru.same_index(*host.phase_index_entries(hidx), off, entries)
        case["results"] = []
        for i, q in enumerate(case["queries"]):
            got = reference_result(case, q, read_alignments(lines, reads), oriented, ident)   # (a fresh mapping: the call adds keys)
            ref = got[0] if isinstance(got, tuple) else got
            d = ru.definition(case, q, m)
            ref["b_reads"] = d["b_reads"]
            ru.same_result(d, ref, "%s q%d (definition)" % (name, i))
            ru.same_result(ru.query_source(host, hidx, q), ref, "%s q%d (HostIndex)" % (name, i))
            if isinstance(got, tuple):
                # pack_bubble accepts what the reference returned: the same bubble as bubble_from_relevant, up to numbering
                packed = phasing.pack_bubble([], [[set(), set()]], got[1])
                assert sorted(packed.overlap_max.tolist()) == sorted(ref["overlap_max"]) and len(packed.aln_b) == len(ref["aln_y"])
            case["results"].append(ref)
            print("%-8s q%-2d %5d aligning, %4d spanning, fell back %d, %5d relevant, %5d alignments, n_b %4d" % (
                name, i, len(ref["cur_aligning"]), ref["n_spanning"], ref["fell_back"], len(ref["rel_reads"]), len(ref["aln_y"]),
                len(ref["b_reads"])))
        # the reference's get_relevant_read_info alone, on the case's widest query
        q = max(case["queries"], key=lambda q: len(q["cur_graph"]) + len(q["prev_graph"]))
        al = read_alignments(lines, reads)
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            reference_result(case, q, al, oriented, ident)
            times.append((time.perf_counter() - t0) * 1e3)
        timings[name + ".relevant_ms"] = sorted(times)[2]
        cases.append(case)
    situations(cases)
    ru.save_golden({"cases": cases, "reference_host_ms": timings})
    for k, v in timings.items():
        print("%-28s %.3f ms" % (k, v))
    print("%d cases, %d queries, %d bytes" % (len(cases), sum(len(c["queries"]) for c in cases), os.path.getsize(ru.GOLDEN_FILE)))


def situations(cases):
    """What the cases must hold, on the reference's numbers."""
    by = {c["name"]: c for c in cases}
    w = by["writes"]
    ent = {(x, b): (a0, a1, s) for x in range(2 * w["n_seg"]) for b, a0, a1, s in
           list(zip(w["index_b"], w["index_a0"], w["index_a1"], w["index_seq"]))[w["index_off"][x]:w["index_off"][x + 1]]}
    assert ent[(0, 2)] == (22, 32, 17) and ent[(2, 0)] == (21, 31, 16)      # the later (b, a) row replaced both keys
    assert ent[(4, 6)] == (8, 80, 7) and ent[(6, 4)] == (7, 70, 6)
    assert ent[(8, 8)] == (2, 9, 9)                                         # the self row leaves (bstart, bend)
    assert ent[(10, 12)][:2] == (1, 2) and ent[(11, 12)][:2] == (5, 6)      # x+ and x-
    r0 = w["results"][0]
    i14 = r0["rel_reads"].index(14)
    assert 14 in r0["cur_aligning"] and r0["aln_off"][i14] == r0["aln_off"][i14 + 1]   # no row at all: relevant, no alignments
    b = by["bubble"]
    r = b["results"]
    assert r[0]["aln_y"] == [10, 20, 12, 22, 24, 24] and 30 not in r[0]["aln_y"] and 32 not in r[0]["aln_y"]   # entrance, exit, downstream dropped
    assert r[0]["overlap_max"] == [200, 90, 200] and r[1]["overlap_max"] == [200, 90, 200]     # the MergedReads pred yields len(read)
    assert r[2]["overlap_max"] == [130, 80, 200] and r[3]["overlap_max"] == [0, -50, 200] and r[4]["overlap_max"][2] == -200
    assert r[5]["overlap_max"] == [200, 90, 200] and r[6]["overlap_max"] == r[7]["overlap_max"] == [130, 70, 200]
    assert r[8]["rel_reads"] == [40, 52] and r[8]["overlap_max"] == [200, 16]
    assert all(r[9][k] == r[2][k] for k in ru.RESULT_KEYS)                                     # duplicates count once
    assert all(not r[i]["cur_aligning"] and not r[i]["b_reads"] for i in (10, 11))
    assert (r[12]["fell_back"], len(r[12]["rel_reads"])) == (0, 0) and (r[13]["fell_back"], len(r[13]["rel_reads"])) == (1, 10)
    assert (r[14]["n_spanning"], r[14]["fell_back"]) == (3, 0) and (r[15]["n_spanning"], r[15]["fell_back"]) == (3, 1)
    assert r[15]["b_reads"] == [20, 22, 24, 26] and r[14]["b_reads"] == [10, 12, 20, 22, 24, 26]
    d = by["degrees"]
    deg = [d["index_off"][x + 1] - d["index_off"][x] for x in range(2 * d["n_seg"])]
    assert set(ru.HUB_DEGREES) <= set(deg) and (2 * d["n_seg"]) % 64 and (2 * by["ids"]["n_seg"]) % 64
    assert max(d["results"][1]["aln_off"][i + 1] - d["results"][1]["aln_off"][i] for i in range(6)) > 1000
    for x in (31, 32, 33, 63, 64, 65, 133):
        r = by["ids"]["results"][0]
        assert x in r["cur_aligning"] and x in r["rel_reads"] and x in r["b_reads"] and x in r["aln_y"]


def time_large_builds():
    """--timings: the reference's dict build on the rows of the cfg2_1k golden and on the union of tests/test_gpu_relevant.py,
    on a host core (what tools/relevant_probe.py measures on the device).  Nothing is saved."""
    import numpy as np
    with np.load(os.path.join(HERE, "cfg2_1k.npz")) as z:
        big = {"n_seg": int(z["n_oriented"]) // 2, "rows_flat": z["rows"].astype(np.int64).reshape(-1)}
    cases = [spec() for spec in ru.SPECS.values()]
    per_copy = sum(len(ru.rows_of(c)) for c in cases)
    lengths, rows, _ = ru.union_case(cases, -(-530000 // per_copy))
    for name, case in (("cfg2_1k", big), ("union", {"n_seg": len(lengths), "rows_flat": rows.reshape(-1)})):
        reads = {"s%d" % i: Read("s%d" % i, 1000) for i in range(case["n_seg"])}
        lines = list(e_lines(case))
        t0 = time.perf_counter()
        read_alignments(lines, reads)
        print("%-8s %7d rows: the reference's dict build takes %.2f s" % (name, len(lines), time.perf_counter() - t0))


if __name__ == "__main__":
    time_large_builds() if "--timings" in sys.argv[1:] else main()
