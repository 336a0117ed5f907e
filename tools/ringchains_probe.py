#!/usr/bin/env python3
"""Developer probe: po_layout_bubblechains_all over repeated calls, from one process on the GPU -- ms_total beside
po_layout_superbubbles_all's on the same graph result in the same process, the stage's own share (ms_chains + ms_label), the
rounds of the ring election -- what DESIGN.md section 3.9u records.

    python tools/ringchains_probe.py [--repeat 21]  the graphs of the table of section 3.9t (the ring of 1 025 nodes, a ring of
                                                    340 diamonds rooted at an interior node, the union of all 4 096 loop-free
                                                    digraphs on 4 nodes, the union of 2 000 random strongly connected digraphs:
                                                    tests/cyclic_utils.py) and the cleaned (b) and merged (c) graph of cfg2_1k
"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

COUNTS = ("n_bubbles", "n_top", "n_chains", "n_ring_chains", "n_ring_bubbles", "n_cyclic_bubbles", "max_chain_bubbles", "n_ring_rounds",
          "n_chain_rounds", "n_nest_rounds", "n_root_runs", "n_split_levels", "n_batches")


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(call, stats, repeat):
    """``repeat`` calls: the last stats and the spread of the wall time, of every ms_* and of the stage's own share."""
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
        if "ms_chains" in last:
            samples.setdefault("ms_own", []).append(last["ms_chains"] + last["ms_label"])
    return last, {k: spread(v) for k, v in samples.items()}


def probe(ov, g, n_order, repeat):
    last, times = measure(lambda: ov.layout_bubblechains_all(g, 1, n_order), ov.bubblechain_all_stats, repeat)
    _, first = measure(lambda: ov.layout_superbubbles_all(g, n_order), ov.superbubble_all_stats, repeat)
    return {"n_nodes": n_order, "n_edges": len(g), "chains_all": {k: last[k] for k in COUNTS}, "chains_all_ms": times,
            "superbubbles_all_ms": first}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=21, help="calls per graph; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    import cyclic_utils as cy
    import partition_utils as pu
    ids = [2 * i for i in range(1025)]
    o_d, e_d = cy.ring_of_diamonds(340)
    graphs = [("ring_1025", ids, pu._ring(ids)), ("ring_of_340_diamonds_interior_lowest", [o_d[1], o_d[0]] + o_d[2:], e_d),
              ("four_node_digraphs_4096",) + cy.four_node_union(), ("strong_union_2000",) + cy.strong_union()]
    out = {"repeat": max(1, args.repeat)}
    for name, order, edges in graphs:
        ov = ExactOverlapper(device=0)
        for i in range((max(list(order) + [-2]) + 2) // 2):
            ov.add_segment("s%d" % i, 1000)
        uv = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        g = ov.graph_from_edges(np.concatenate([uv, np.full((len(uv), 2), 1)], axis=1), order)
        out[name] = probe(ov, g, len(order), args.repeat)
        g.free()
        ov.close()
    from test_gpu_merge import BY_NAME, cleaned, edges_from_text   # (the graphs of a text case, as the tests rebuild them)
    with tempfile.TemporaryDirectory() as tmp:
        ov, edges_res = edges_from_text(BY_NAME["reduced_cfg2_1k"], pathlib.Path(tmp))
        final = cleaned(ov, edges_res)
        merged = ov.layout_merge(final)
        for tag, g in (("cfg2_1k_cleaned", final), ("cfg2_1k_merged", merged)):
            out[tag] = probe(ov, g, len(g.node_order()), args.repeat)
        for r in (merged, final, edges_res):
            r.free()
        ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
