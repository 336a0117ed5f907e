#!/usr/bin/env python3
"""Developer probe: the statistics of po_layout_superbubbles_all (split nodes and levels, rootless SCCs, root runs, the ms_* of
every phase and the wall time of the call) over repeated calls, from one process on the GPU, and next to each the times of
po_layout_superbubbles on the same graph result in the same process -- what DESIGN.md section 3.9t records.

    python tools/cyclic_probe.py [--repeat 21]      the ring of 1 025 nodes, a ring of 340 diamonds rooted at an interior node,
                                                    K8 in both directions, the union of all 4 096 loop-free digraphs on 4
                                                    nodes and the union of 2 000 random strongly connected digraphs
                                                    (tests/cyclic_utils.py)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

COUNTS = ("n_bubbles", "n_cyclic_bubbles", "n_split", "n_split_levels", "n_rootless", "n_root_runs", "n_certified", "n_edge_filtered",
          "n_scc_rounds", "n_batches")


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(call, stats, repeat):
    """``repeat`` calls: the last stats and the spread of the wall time and of every ms_*."""
    samples, last = {}, None
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        call()
        wall = 1e3 * (time.perf_counter() - t0)
        last = stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        samples.setdefault("ms_wall", []).append(wall)
        for k, v in last.items():
            if k.startswith("ms_"):
                samples.setdefault(k, []).append(v)
    return last, {k: spread(v) for k, v in samples.items()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    import cyclic_utils as cy
    import partition_utils as pu
    ids = [2 * i for i in range(1025)]
    o_d, e_d = cy.ring_of_diamonds(340)
    k8 = ids[:8]
    graphs = [("ring_1025", ids, pu._ring(ids)), ("ring_of_340_diamonds_interior_lowest", [o_d[1], o_d[0]] + o_d[2:], e_d),
              ("k8_both_directions", k8, [(u, v) for u in k8 for v in k8 if u != v]),
              ("four_node_digraphs_4096",) + cy.four_node_union(), ("strong_union_2000",) + cy.strong_union()]
    out = {"repeat": max(1, args.repeat)}
    for name, order, edges in graphs:
        ov = ExactOverlapper(device=0)
        for i in range((max(list(order) + [-2]) + 2) // 2):
            ov.add_segment("s%d" % i, 1000)
        uv = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        g = ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 2), 1)], axis=1), order)
        n_order = len(order)
        last, times = measure(lambda: ov.layout_superbubbles_all(g, n_order), ov.superbubble_all_stats, args.repeat)
        old, old_times = measure(lambda: ov.layout_superbubbles(g, n_order), ov.superbubble_stats, args.repeat)
        out[name] = {"n_nodes": n_order, "n_edges": len(uv), "all": {k: last[k] for k in COUNTS}, "all_ms": times,
                     "acyclic_only": {"n_bubbles": old["n_bubbles"], "n_batches": old["n_batches"]}, "acyclic_only_ms": old_times}
        g.free()
        ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
