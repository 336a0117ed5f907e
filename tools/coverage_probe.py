#!/usr/bin/env python3
"""Developer probe: the config-2 read set through overlap -> layout stage 1 -> the four cleaning calls -> merge, once, on
the GPU, and from that one process the statistics of po_layout_coverage (n_pairs, max_set and the ms_* of its two phases)
over repeated calls on the merged graph and on the stage-1 graph -- what DESIGN.md section 3.9f records.

    python tools/coverage_probe.py [--config cfg2] [--repeat 11] [--graph merged|stage1|both]

Run each graph as a step of its own (``--graph merged``, then ``--graph stage1``) where a step has a time limit.
The point of comparison is the reference's loop on a host core: tests/golden/make_coverage_golden.py --time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, graph, rows, repeat):
    samples, last = {}, None
    for i in range(max(1, repeat) + 1):
        ov.layout_coverage(graph, rows)
        last = ov.coverage_stats()
        if i == 0:
            continue                                             # (one pass outside the samples: the workspaces grow here)
        for k, v in last.items():
            if k.startswith("ms_"):
                samples.setdefault(k, []).append(v)
    return {"stats": last, "ms": {k: spread(v) for k, v in samples.items()}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="cfg2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=11, help="calls per graph; medians, minima and maxima are reported")
    ap.add_argument("--graph", default="both", choices=("merged", "stage1", "both"))
    args = ap.parse_args(argv)
    ov = ExactOverlapper(device=0)
    for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
        ov.add_sequence(name, seq)
    rows = ov.overlaps_result(args.min_length)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    out = {"graph": args.config, "repeat": max(1, args.repeat), "n_rows": len(rows), "n_edges_stage1": len(edges)}
    if args.graph in ("stage1", "both"):
        out["stage1"] = measure(ov, edges, rows, args.repeat)
    if args.graph in ("merged", "both"):
        cur = edges
        for call in (lambda r: ov.layout_reduce(r, 1000), lambda r: ov.layout_tips(r, 4, 5000), ov.layout_diamonds,
                     lambda r: ov.layout_tips(r, 4, 5000)):
            nxt = call(cur)
            if cur is not edges:
                cur.free()
            cur = nxt
        merged = ov.layout_merge(cur)
        out["n_edges_merged"] = len(merged)
        out["merged"] = measure(ov, merged, rows, args.repeat)
        merged.free()
        cur.free()
    edges.free()
    rows.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
