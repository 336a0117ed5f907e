#!/usr/bin/env python3
"""Generate tests/golden/coverage_cases.npz by EXECUTING the reference's own function.

Runs only where the reference checkout is present (/root/reference); the output is committed.

    phasm.assembly_graph.average_coverage_path(g, read_alignments, [u, v])   phasm/assembly_graph.py:544-591, assembler.py:190-193

run unmodified, for every edge, on the stand-in graph of make_merge_golden:
  (a) on the stage-1 graph of every text case of merge_cases.npz and of the seeded cases of tests/coverage_utils.py,
  (b) on that graph after the whole cleaning chain of assembler.py:145-182 at the CLI defaults and merge_unambiguous_paths.
``read_alignments`` is filled as assembler.py:65-76 fills it: from the LocalAlignment that the reference's gfa2_line_to_la
makes of EVERY E line, before any filter.

The restatements of tests/coverage_utils.py (the plain statement and the device's scheme) must equal the reference's
integers and quotients on every application here (asserted below), and every situation the seeded cases aim at must occur.

    --time    also print what the reference's loop takes on the largest case, on this host core"""
import io
import os
import sys
import time
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_merge_golden as mmg  # noqa: E402  (sets the paths up and installs the stand-in graph; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import coverage_utils as cu  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import reduce_utils as ru  # noqa: E402
import tips_utils as tu  # noqa: E402

TIME = "--time" in sys.argv


def record_alignments(text):
    """assembler.py:65-76 on every E line of the text."""
    reads = rgfa.gfa2_parse_segments(io.StringIO(text))
    read_alignments = defaultdict(dict)
    for la in map(rgfa.gfa2_line_to_la(reads), (l for l in io.StringIO(text) if l.startswith("E"))):
        a_read, b_read = la.get_oriented_reads()
        read_alignments[a_read][b_read] = la
        read_alignments[b_read][a_read] = la.switch()
    return read_alignments


def run_coverage(g, read_alignments, node_index, n_ids, rows, lengths, stage, totals):
    """average_coverage_path for every edge of g.  Returns the record of this application and the loop's seconds."""
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}

    def idx(n):
        return n_ids + k_of[str(n)] if isinstance(n, MergedReads) else node_index[str(n)]

    members = {n_ids + k: [node_index[str(r)] for r in n.reads] for k, n in enumerate(merged)}
    all_len = [int(x) for x in lengths] + [len(n) for n in merged]
    t0 = time.perf_counter()
    cov = {(u, v): ag.average_coverage_path(g, read_alignments, [u, v]) for u, v in g.edges_iter()}
    seconds = time.perf_counter() - t0
    e = mdg.edge_array(g, idx)
    e = e[tu.by_uv(e)]
    by_idx = {(idx(u), idx(v)): c for (u, v), c in cov.items()}
    avg = np.asarray([by_idx[(u, v)] for u, v in e[:, :2].tolist()], dtype=np.float64)
    counts = cu.new_counts()
    s1, p1, q1 = cu.edge_coverage(rows, e, members, all_len)
    s2, p2, q2 = cu.edge_coverage_by_sets(rows, e, members, all_len, counts)
    assert np.array_equal(s1, s2) and np.array_equal(p1, p2), "the two restatements differ"
    assert q1.tobytes() == avg.tobytes() and q2.tobytes() == avg.tobytes(), "a restatement differs from the reference"
    n_nodes, n_pairs, max_set = cu.set_stats(rows, e, members)
    counts["merged_self_loops"] = int(((e[:, 0] == e[:, 1]) & (e[:, 0] >= n_ids)).sum())
    counts["path_over_64_members"] = sum(len(m) > 64 for m in members.values())
    counts["set_over_1024_reads"] = int(max_set > 1024)
    counts["sum_over_2_32"] = int((s1 >= 2**32).sum())
    counts["path_length_over_2_31"] = int((p1 >= 2**31).sum())
    for k, v in counts.items():
        totals[k] += v
    totals["applications"] += 1
    rec = {"stage": stage, "n_ids": n_ids, "n_edges": len(e), "n_nodes": n_nodes, "n_pairs": n_pairs, "max_set": max_set,
           "u": e[:, 0], "v": e[:, 1], "read_length_sum": s1, "path_length": p1, "avg_coverage": avg}
    return rec, seconds


def text_case(c, totals):
    name, params = c["name"], c["params"]
    text = cu.case_text(c)
    out = {k: c[k] for k in ("reduce_case", "synth", "text_sha256") if k in c}
    out.update(name=name, params=params, results=[])
    read_alignments = record_alignments(text)
    from phasm_amd.io import gfa as my_gfa
    _, seg_len, rows = my_gfa.read_gfa2_rows(text.splitlines(True))
    g, node_index = mrg.stage1_graph(text, params)
    n_ids = len(node_index)
    assert n_ids == 2 * len(seg_len)
    lengths = np.repeat(seg_len, 2)
    in_graph = set(node_index[str(n)] for n in g)
    # the situations of the rows, as the reference's stage 1 left them
    A = cu.aligning_reads(rows)
    edges1 = set((node_index[str(u)], node_index[str(v)]) for u, v in g.edges_iter())
    pairs = [tuple(r) for r in rows[:, :2].tolist()]
    totals["contained_read_counts"] += sum(1 for n in in_graph for y in A.get(n, ()) if y not in in_graph)
    totals["dropped_row_counts"] += sum(1 for a, b in pairs if a in in_graph and b in in_graph and a != b and
                                        (a, b) not in edges1 and (b, a) not in edges1)
    distinct = set(pairs)
    totals["one_strand_only"] += sum(1 for a, b in distinct if (b ^ 1, a ^ 1) not in distinct and a in in_graph and b in in_graph)
    totals["duplicate_rows"] += len(pairs) - len(distinct)
    totals["self_row"] += sum(1 for a, b in pairs if a == b and a in in_graph)
    zero = [n for n in range(n_ids) if lengths[n] == 0]
    totals["zero_length_segments"] += len(zero)
    assert not any(n in in_graph for n in zero), "stage 1 emitted an edge at a segment of length 0"
    rec, sec_a = run_coverage(g, read_alignments, node_index, n_ids, rows, lengths, "a", totals)
    out["results"].append(rec)
    # the chain, assembler.py:145-182, the merge, then (b)
    g, node_index = mrg.stage1_graph(text, params)
    g.remove_edges_from(ag.remove_transitive_edges(g, du.STAGE_FUZZ))
    ag.make_symmetric(g)
    ag.remove_tips(g, du.STAGE_L, du.STAGE_B)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    ag.remove_diamond_tips(g)
    ag.remove_tips(g, du.STAGE_L)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    ag.merge_unambiguous_paths(g)
    rec, seconds = run_coverage(g, read_alignments, node_index, n_ids, rows, lengths, "b", totals)
    out["results"].append(rec)
    a = out["results"][0]
    print("%-30s rows %6d  a: %6d edges, %6d pairs, largest set %5d  b: %5d edges, %6d pairs, largest set %5d%s" % (
        name, len(rows), a["n_edges"], a["n_pairs"], a["max_set"], rec["n_edges"], rec["n_pairs"], rec["max_set"],
        "  reference: a %.1f ms, b %.1f ms" % (1e3 * sec_a, 1e3 * seconds) if TIME else ""))
    return out, max(sec_a, seconds), len(rows), a["n_edges"]


def main():
    totals = dict(cu.new_counts(), applications=0)
    cases, slowest = [], (0.0, None, 0, 0)
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            out, sec, n_rows, n_edges = text_case(c, totals)
            cases.append(out)
            slowest = max(slowest, (sec, c["name"], n_rows, n_edges))
    for synth in cu.NEW_CASES:
        src = {"name": "_".join(str(v) for v in synth.values()), "params": ru.DEFAULT_PARAMS, "synth": synth}
        src["text_sha256"] = ru.text_digest(cu.case_text(src))
        out, sec, n_rows, n_edges = text_case(src, totals)
        cases.append(out)
        slowest = max(slowest, (sec, src["name"], n_rows, n_edges))
    for k in cu.SITUATIONS:
        assert totals[k] > 0, "situation %s never occurs" % k
    cu.save_golden({"situation_totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", cu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(cu.GOLDEN_FILE), "bytes")
    if TIME:
        print("the reference's loop, slowest application: %.1f ms on %s (%d rows, %d stage-1 edges)" % (
            1e3 * slowest[0], slowest[1], slowest[2], slowest[3]))


if __name__ == "__main__":
    main()
