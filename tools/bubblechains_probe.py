#!/usr/bin/env python3
"""Developer probe: the statistics of po_layout_bubblechains (chains, rounds per loop, batches, the ms_* of every phase and
the wall time of the call) over repeated calls, from one process on the GPU -- what DESIGN.md section 3.9k records.

    python tools/bubblechains_probe.py [--repeat 21]           the direct cases of tests/bubblechain_utils.py that the section
                                                               names (the empty graph, the paths of 1 025 nodes, nesting
                                                               depth 300) and the text case reduced_cfg2_1k of
                                                               tests/golden/merge_cases.npz at (b) cleaned and (c) merged
    python tools/bubblechains_probe.py --config cfg2           a config of phasm_amd.synth through overlap -> layout -> merge

The point of comparison is the reference's build_bubblechains on a host core: tests/golden/make_bubblechains_golden.py --time.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

ROUNDS = ("n_nest_rounds", "n_chain_rounds", "n_batches")


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, graph, repeat):
    """``repeat`` calls on one graph result: the last stats, the spread of the times and of the rounds."""
    n_order = len(graph.node_order())
    samples, last = {}, None
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        ov.layout_bubblechains(graph, 1, n_order)
        wall = 1e3 * (time.perf_counter() - t0)
        last = ov.bubblechain_stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        samples.setdefault("ms_wall", []).append(wall)
        for k, v in last.items():
            if k.startswith("ms_") or k in ROUNDS:
                samples.setdefault(k, []).append(v)
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}}


def cleaned_and_merged(ov, rows, args):
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
    out = {"n_edges_stage1": len(edges), "b_cleaned": measure(ov, cur, args.repeat), "c_merged": measure(ov, merged, args.repeat)}
    for r in (merged, cur, edges):
        r.free()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default=None, choices=sorted(synth.CONFIGS))
    ap.add_argument("--text-case", default="reduced_cfg2_1k")
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--length-fuzz", type=int, default=1000)
    ap.add_argument("--max-tip-length", type=int, default=4)
    ap.add_argument("--max-tip-length-bases", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    out = {"repeat": max(1, args.repeat)}
    if args.config is not None:
        ov = ExactOverlapper(device=0)
        for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
            ov.add_sequence(name, seq)
        out[args.config] = cleaned_and_merged(ov, ov.overlaps_result(args.min_length), args)
        ov.close()
        print(json.dumps(out))
        return 0
    import merge_utils as mu
    import bubblechain_utils as bu
    for name, order, edges, n_ids, _ in bu.direct_inputs():
        if not (name == "empty" or name.startswith("sb_path_1025") or name == "bc_nesting_depth_300"):
            continue
        ov = ExactOverlapper(device=0)
        for i in range((max(list(order) + [-2]) + 2) // 2):
            ov.add_segment("s%d" % i, 1000)
        uv = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        g = ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 2), 1)], axis=1), order)
        out[name] = measure(ov, g, args.repeat)
        g.free()
        ov.close()
    case = next(c for c in mu.load_golden()["cases"] if c["name"] == args.text_case)
    ov = ExactOverlapper(device=0)
    with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
        f.write(mu.case_text(case))
        f.flush()
        _, rows = ov.add_gfa(f.name)
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    cur = edges_res
    import diamond_utils as du
    import tips_utils as tu
    for call in (lambda r: ov.layout_reduce(r, du.STAGE_FUZZ), lambda r: ov.layout_tips(r, du.STAGE_L, du.STAGE_B),
                 ov.layout_diamonds, lambda r: ov.layout_tips(r, du.STAGE_L, tu.DEFAULT_B)):
        nxt = call(cur)
        if cur is not edges_res:
            cur.free()
        cur = nxt
    merged = ov.layout_merge(cur)
    out[args.text_case] = {"b_cleaned": measure(ov, cur, args.repeat), "c_merged": measure(ov, merged, args.repeat)}
    for r in (merged, cur, edges_res):
        r.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
