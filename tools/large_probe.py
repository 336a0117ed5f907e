#!/usr/bin/env python3
"""Time po_phase_large on bubbles of 65, 4 097 and 32 769 listed paths (6, 12 and 15 diamonds in series and an arm:
tests/paths_utils.py ``many_paths``) at R = 100 and R = 2 000 relevant reads: median, minimum and maximum of 21 calls, each as
the whole call through ``DevicePaths.score_large`` (host packing, uploads, four stages, the copy of the best list) and as the
device time of ``large_stats()``.  With ``--reference`` (where the reference checkout is) also the reference's
``phase_large_bubble`` on one host core for the same bubbles -- the comparison on record: nothing else here scores them.

    python tools/large_probe.py [--calls 21] [--reference /path/to/reference] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import large_utils as lu  # noqa: E402
import paths_utils as pp  # noqa: E402


def reference_seconds(ref_root, order, edges, rel, reads_of, entrance, exit_):
    sys.path.insert(0, ref_root)
    import networkx
    from phasm.alignments import LocalAlignment, OrientedRead, Read
    from phasm.phasing import BubbleChainPhaser
    from phasm.typing import RelevantReadInfo
    read = {}
    oriented = lambda r: read.setdefault(int(r), OrientedRead(Read("g%d" % r, 1000), "+"))   # noqa: E731
    node = {n: oriented(reads_of(n)[0]) for n in order}
    g = networkx.DiGraph()
    g.add_nodes_from(node[n] for n in order)
    for u, v, w in edges:
        g.add_edge(node[u], node[v], weight=w)
    info = {}
    for r in range(len(rel.rel_reads)):
        a = OrientedRead(Read("rel%d" % r, 1000), "+")
        lo, hi = int(rel.aln_off[r]), int(rel.aln_off[r + 1])
        info[a] = RelevantReadInfo({LocalAlignment(a, oriented(rel.b_reads[x]), (int(a0), int(a1)), (0, int(a1 - a0)))
                                    for x, a0, a1 in zip(rel.aln_b[lo:hi], rel.aln_a0[lo:hi], rel.aln_a1[lo:hi])}, int(rel.overlap_max[r]))
    ph = object.__new__(BubbleChainPhaser)
    ph.ploidy = 2
    t0 = time.perf_counter()
    paths = [tuple(p) for p in networkx.all_simple_paths(g, node[entrance], node[exit_])]
    ph.phase_large_bubble(paths, info)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = []
    for k in (6, 12, 15):
        edges = [list(e) for e in pp._w(pp.many_paths(k))]
        order = pp.first_seen(edges)
        ov, g = lu.device_graph(order, edges)
        paths = ov.phase_paths_resident(g, 1 << 20)
        g.free()
        for R in (100, 2000):
            rel, reads_of = lu.simple_rel(paths.interior_of(0), R, 11)
            paths.score_large(0, rel, reads_of, 2)                    # (the buffers of the call are allocated here)
            whole, device, stages = [], [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                paths.score_large(0, rel, reads_of, 2)
                whole.append((time.perf_counter() - t0) * 1e3)
                st = paths.large_stats()
                device.append(st["ms_total"])
                stages.append((st["ms_intervals"], st["ms_score"], st["ms_best"]))
            row = {"n_paths": int(paths.bubbles["n_paths"][0]), "n_reads": R, "n_inside": st["n_inside"], "calls": args.calls,
                   "call_ms": [statistics.median(whole), min(whole), max(whole)],
                   "device_ms": [statistics.median(device), min(device), max(device)],
                   "stage_ms_median": [statistics.median(s[j] for s in stages) for j in range(3)]}
            if args.reference:
                row["reference_s"] = reference_seconds(args.reference, order, edges, rel, reads_of, int(paths.bubbles["entrance"][0]),
                                                       int(paths.bubbles["exit"][0]))
            out.append(row)
            print("P %6d R %5d: call %.3f ms (%.3f .. %.3f), device %.3f ms (%.3f .. %.3f); intervals %.3f score %.3f best %.3f%s" % (
                row["n_paths"], R, *row["call_ms"], *row["device_ms"], *row["stage_ms_median"],
                "; reference %.2f s" % row["reference_s"] if args.reference else ""), flush=True)
        paths.close()
        ov.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
