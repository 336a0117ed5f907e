#!/usr/bin/env python3
"""Developer probe: the statistics of po_phase_paths (bubbles, listed paths, counting rounds, batches, the ms_* of every phase
and the wall time of the call, the copy of the result to the host included) over repeated calls, from one process on the GPU
-- what DESIGN.md section 3.9r records.

    python tools/paths_probe.py [--repeat 21] [--max-paths 10]     the paths of 1 025 nodes of tests/superbubble_utils.py (1 024 bare
                                                                   bubbles), the text case reduced_cfg2_1k of
                                                                   tests/golden/merge_cases.npz at (b) cleaned and (c) merged, a
                                                                   bubble of 10 paths and one of 2^15 + 1 (both listed in full)

Next to each: what networkx.all_simple_paths (on the bubbles with at most max-paths paths) and a breadth-first
superbubble_nodes take on the same graph and the same bubbles on a host core (best of 5), where networkx is installed.
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

ROUNDS = ("n_count_rounds", "n_batches")


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def host_side(graph, bp, max_paths):
    """networkx.all_simple_paths and a breadth-first superbubble_nodes on every bubble of ``bp``: seconds, best of 5."""
    try:
        import networkx
    except ImportError:
        return None
    g = networkx.DiGraph()
    g.add_nodes_from(graph.node_order().tolist())
    g.add_edges_from((int(r["u"]), int(r["v"])) for r in graph.rows())
    bubbles = [(int(r["entrance"]), int(r["exit"]), int(r["n_paths"])) for r in bp.bubbles]
    runs, n_paths, n_skipped = [], 0, 0
    for _ in range(5):
        t0 = time.perf_counter()
        n_paths, n_skipped = 0, 0
        for s, t, count in bubbles:
            if count <= max_paths:
                n_paths += sum(1 for _ in networkx.all_simple_paths(g, s, t))
            else:
                n_skipped += 1
            seen, todo = {s, t}, [s]
            while todo:
                nxt = []
                for v in todo:
                    for w in g.successors(v):
                        if w not in seen:
                            seen.add(w)
                            nxt.append(w)
                todo = nxt
        runs.append(time.perf_counter() - t0)
    return {"ms_best_of_5": round(1e3 * min(runs), 4), "paths_enumerated": n_paths, "bubbles_not_enumerated": n_skipped}


def measure(ov, graph, repeat, max_paths):
    """``repeat`` calls on one graph result: the last stats, the spread of the times and of the rounds."""
    samples, last, bp = {}, None, None
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        bp = ov.phase_paths(graph, max_paths)
        wall = 1e3 * (time.perf_counter() - t0)
        last = ov.paths_stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        samples.setdefault("ms_wall", []).append(wall)
        for k, v in last.items():
            if k.startswith("ms_") or k in ROUNDS:
                samples.setdefault(k, []).append(v)
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}, "networkx": host_side(graph, bp, max_paths)}


def direct(order, edges, repeat, max_paths):
    ov = ExactOverlapper(device=0)
    for i in range((max(list(order) + [-2]) + 2) // 2):
        ov.add_segment("s%d" % i, 1000)
    uv = np.asarray([e[:2] for e in edges], dtype=np.int64).reshape(-1, 2)
    g = ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 2), 1)], axis=1), order)
    out = measure(ov, g, repeat, max_paths)
    g.free()
    ov.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--text-case", default="reduced_cfg2_1k")
    ap.add_argument("--max-paths", type=int, default=10, help="as `phasm phase -b` (default: 10)")
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    out = {"repeat": max(1, args.repeat), "max_paths": args.max_paths}
    import diamond_utils as du
    import merge_utils as mu
    import paths_utils as pp
    import superbubble_utils as su
    import tips_utils as tu
    for name, order, edges, _ in su.direct_inputs():
        if name.startswith("sb_path_1025"):
            out[name] = direct(order, edges, args.repeat, args.max_paths)
    fan = [(0, 2 + i) for i in range(10)] + [(2 + i, 1) for i in range(10)]
    out["one_bubble_10_paths"] = direct(pp.first_seen(fan), fan, args.repeat, 10)
    big = pp.many_paths(15)
    out["one_bubble_32769_paths"] = direct(pp.first_seen(big), big, args.repeat, 1 << 16)
    case = next(c for c in mu.load_golden()["cases"] if c["name"] == args.text_case)
    ov = ExactOverlapper(device=0)
    with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
        f.write(mu.case_text(case))
        f.flush()
        _, rows = ov.add_gfa(f.name)
    edges_res, _ = ov.layout_edges(rows, **case["params"])
    rows.free()
    cur = edges_res
    for call in (lambda r: ov.layout_reduce(r, du.STAGE_FUZZ), lambda r: ov.layout_tips(r, du.STAGE_L, du.STAGE_B),
                 ov.layout_diamonds, lambda r: ov.layout_tips(r, du.STAGE_L, tu.DEFAULT_B)):
        nxt = call(cur)
        if cur is not edges_res:
            cur.free()
        cur = nxt
    merged = ov.layout_merge(cur)
    out[args.text_case] = {"b_cleaned": measure(ov, cur, args.repeat, args.max_paths), "c_merged": measure(ov, merged, args.repeat, args.max_paths)}
    for r in (merged, cur, edges_res):
        r.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
