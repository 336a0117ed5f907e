#!/usr/bin/env python3
"""Developer probe: the statistics of po_layout_contigs (contigs, rounds per loop, batches, the ms_* of every phase and the wall
time of the call) over repeated calls, from one process on the GPU -- what DESIGN.md section 3.9l records.

    python tools/contigs_probe.py [--repeat 21]       the direct cases of tests/contig_utils.py that the section names (the empty
                                                      graph, the paths of 1 025 nodes, the comb of 300 late starts), each with the
                                                      chains built by the call and with an exclude set given (nothing excluded),
                                                      and the text case reduced_cfg2_1k of tests/golden/merge_cases.npz at (b)
                                                      cleaned and (c) merged

The point of comparison is the reference's identify_contigs on a host core: tests/golden/make_contigs_golden.py --time.
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

from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

ROUNDS = ("n_path_rounds", "n_cover_rounds", "n_batches")


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, graph, repeat, min_len, given):
    """``repeat`` calls on one graph result: the last stats, the spread of the times and of the rounds.  ``given``: with an
    exclude set from the caller (nothing excluded) instead of the chains the call builds itself."""
    n_order = len(graph.node_order())
    exclude = np.zeros(n_order, dtype=np.uint8) if given else None
    samples, last = {}, None
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        ov.layout_contigs(graph, min_len, 1, exclude, n_order)
        wall = 1e3 * (time.perf_counter() - t0)
        last = ov.contig_stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        samples.setdefault("ms_wall", []).append(wall)
        for k, v in last.items():
            if k.startswith("ms_") or k in ROUNDS:
                samples.setdefault(k, []).append(v)
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}}


def both(ov, graph, repeat, min_len):
    return {"own_chains": measure(ov, graph, repeat, min_len, False), "exclude_given": measure(ov, graph, repeat, min_len, True)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--text-case", default="reduced_cfg2_1k")
    ap.add_argument("--min-contig-len", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    out = {"repeat": max(1, args.repeat)}
    import contig_utils as ct
    import merge_utils as mu
    for name, order, edges, lengths, _, min_len in ct.direct_inputs():
        if not (name == "empty" or name.startswith("path_1025") or name == "comb_300"):
            continue
        ov = ExactOverlapper(device=0)
        for i in range((max(list(order) + [-2]) + 2) // 2):
            ov.add_segment("s%d" % i, lengths.get(2 * i, 1))
        e = np.asarray([(u, v, w, 17) for u, v, w in edges], dtype=np.int64).reshape(-1, 4)
        g = ov.graph_from_edges(e, order)
        out[name] = both(ov, g, args.repeat, min_len)
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
    out[args.text_case] = {"b_cleaned": both(ov, cur, args.repeat, args.min_contig_len),
                           "c_merged": both(ov, merged, args.repeat, args.min_contig_len)}
    for r in (merged, cur, edges_res):
        r.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
