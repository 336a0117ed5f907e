#!/usr/bin/env python3
"""Times po_layout_reduce (transitive reduction + symmetry pass) at full size.

    python tools/reduce_probe.py [--configs cfg2,cfg3] [--repeat 9] [--fuzz 1000] [--sample 2000] [--out FILE]

Per config: the reads are generated and uploaded, po_overlaps leaves the rows in HBM, po_layout_edges the stage-1
edges; then po_layout_reduce runs --repeat times on those edges (one warm-up call first: it allocates the handle's
workspaces) and po_reduce_stats of EVERY call is printed with the medians.  Device times are hipEvent pairs around
the four phases; the wall time of the call (which includes the flag-free result hand-over) is printed beside them.

The only CPU baseline that exists on a GPU box is this repository's own Python statement of the contract
(tests/reduce_utils.py), so it is timed on the FIRST --sample nodes of the same graph and labelled as what it is: a
restatement on a sample, not the reference (which needs hours at this size).  A kernel table comes from a run of
its own:  rocprofv3 --kernel-trace --stats -- python tools/reduce_probe.py --configs cfg2 --repeat 3 --sample 0"""
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

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def probe(cfg_name, repeat, fuzz, sample, min_length, emit):
    cfg = synth.CONFIGS[cfg_name]
    ov = ExactOverlapper(device=0)
    for n, s in synth.oriented(synth.generate_reads(cfg)):
        ov.add_sequence(n, s)
    rows = ov.overlaps_result(min_length)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    n_rows = len(rows)
    rows.free()
    lst = ov.layout_stats()
    emit("%s: %d oriented reads, %d rows, %d stage-1 edges (layout %.3f ms), fuzz %d" %
         (cfg_name, len(ov), n_rows, len(edges), lst["ms_total"], fuzz))
    ov.layout_reduce(edges, fuzz).free()          # warm-up: workspaces
    samples = []
    for k in range(repeat):
        t0 = time.perf_counter()
        kept = ov.layout_reduce(edges, fuzz)
        wall = (time.perf_counter() - t0) * 1e3
        st = ov.reduce_stats()
        st["wall_ms"] = wall
        kept.free()
        samples.append(st)
        emit("  call %d: " % k + json.dumps({a: (round(b, 4) if isinstance(b, float) else b) for a, b in st.items()}))
    med = {k: statistics.median(s[k] for s in samples) for k in ("ms_csr", "ms_mark", "ms_symmetric", "ms_emit", "ms_total", "wall_ms")}
    emit("  median of %d: " % repeat + json.dumps({k: round(v, 4) for k, v in med.items()}))
    st = samples[-1]
    emit("  counts: in %d, transitive %d, asymmetric %d, out %d, max out-degree %d" %
         (st["n_edges_in"], st["n_transitive"], st["n_asymmetric"], st["n_edges_out"], st["max_out_degree"]))
    if sample:
        import reduce_utils as ru
        e = edges.rows()
        arr = np.stack([e["u"], e["v"], e["weight"]], 1).astype(np.int64)
        by_src = np.argsort(arr[:, 0], kind="stable")
        start = np.searchsorted(arr[by_src, 0], np.arange(len(ov) + 1))
        nodes = [v for v in range(len(ov)) if start[v + 1] > start[v]][:sample]
        t0 = time.perf_counter()
        n_out = 0
        for v in nodes:
            own = by_src[start[v]:start[v + 1]]
            idx = np.unique(np.concatenate([own] + [by_src[start[w]:start[w + 1]] for w in arr[own, 1].tolist()]))
            ru.reduce_edges(arr[idx], fuzz, rank=idx, nodes=[v])
            n_out += len(own)
        dt = time.perf_counter() - t0
        emit("  CPU, Python restatement of the contract (tests/reduce_utils.py) on a SAMPLE -- the first %d nodes, %d out-edges, "
             "marking only: %.2f s = %.2f ms per node (x %d nodes = %.0f s for the whole graph on one host core)" %
             (len(nodes), n_out, dt, dt / len(nodes) * 1e3, len(ov), dt / len(nodes) * len(ov)))
    edges.free()
    ov.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--fuzz", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for name in args.configs.split(","):
        probe(name, args.repeat, args.fuzz, args.sample, args.min_length, emit)


if __name__ == "__main__":
    main()
