#!/usr/bin/env python3
"""Developer probe: the config-2 read set through overlap -> layout stage 1 -> the four cleaning calls -> the merge, once,
on the GPU, and from that one process the statistics of po_layout_components (rounds, batches and the ms_* of every phase)
over repeated calls on the cleaned graph (stage b) and on the merged graph (stage c) -- what DESIGN.md section 3.9h records.

    python tools/components_probe.py [--config cfg2] [--repeat 21]
    python tools/components_probe.py --lasso N    a ring of N reads with a tail of 8 (tests/merge_utils.py): before the merge
                                                  two paths of N nodes -- the rounds at depth

The point of comparison is networkx on a host core: tests/golden/make_components_golden.py --time.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, graph, repeat):
    """``repeat`` calls on one graph result: the last stats, the spread of the times and of the rounds."""
    n_order = len(graph.node_order())
    samples, last = {}, None
    for i in range(max(1, repeat) + 1):
        ov.layout_components(graph, n_order)
        last = ov.components_stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        for k, v in last.items():
            if k.startswith("ms_") or k == "n_rounds":
                samples.setdefault(k, []).append(v)
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="cfg2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--length-fuzz", type=int, default=1000)
    ap.add_argument("--max-tip-length", type=int, default=4)
    ap.add_argument("--max-tip-length-bases", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    ap.add_argument("--lasso", type=int, default=None, metavar="N")
    args = ap.parse_args(argv)
    ov = ExactOverlapper(device=0)
    if args.lasso is not None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import merge_utils as mu
        import reduce_utils as ru
        what = "lasso_%d" % args.lasso
        with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
            f.write(ru.gfa_text(*mu.lasso_case(args.lasso)))
            f.flush()
            _, rows = ov.add_gfa(f.name)
    else:
        what = args.config
        for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
            ov.add_sequence(name, seq)
        rows = ov.overlaps_result(args.min_length)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    rows.free()
    cur = edges
    for call in (lambda r: ov.layout_reduce(r, args.length_fuzz),
                 lambda r: ov.layout_tips(r, args.max_tip_length, args.max_tip_length_bases),
                 ov.layout_diamonds, lambda r: ov.layout_tips(r, args.max_tip_length, 5000)):
        nxt = call(cur)
        if cur is not edges:
            cur.free()
        cur = nxt
    merged = ov.layout_merge(cur)
    out = {"graph": what, "repeat": max(1, args.repeat), "n_edges_stage1": len(edges),
           "b_cleaned": measure(ov, cur, args.repeat), "c_merged": measure(ov, merged, args.repeat)}
    for r in (merged, cur, edges):
        r.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
