#!/usr/bin/env python3
"""Developer probe: the statistics of po_phase_branch (extensions, kept, survivors, the level used, the ms_* of every phase and
the wall time of the call) over repeated calls, from one process on the GPU -- what DESIGN.md section 3.9n records.

    python tools/phase_probe.py [--repeat 11]     three bubbles from the generator of tests/phase_utils.py (random_case):
        p7_k4_c20_r60       7 paths, ploidy 4, 20 candidate sets, 60 relevant reads: 48 020 extensions
        p10_k4_c500_r100    the defaults of `phasm phase` at their limits: 10 paths, 500 candidates, 5 000 000 extensions
        p10_k2_c50_r2000    few extensions, many reads: the table dominates

Every shape is measured three times: at the command's default threshold 1e-3, where these random bubbles keep little or
nothing (``default_threshold``: the cost of scoring alone); at threshold 0, where EVERY extension is kept, compacted and
copied home (``keep_all``: the most the call can cost); and at threshold 0 with the command's default pruning (factor 0.1,
step 0.1, 500 candidates, 9 rounds: ``keep_all_and_prune``).  The bubble is packed once, outside the timed calls; the wall
time is the whole call from numpy arrays to numpy arrays.

The point of comparison is the reference's BubbleChainPhaser.branch on a host core, which DESIGN.md section 3.9n has for the
first shape.
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

from phasm_amd import phasing  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

SHAPES = {"p7_k4_c20_r60": dict(k=4, P=7, C=20, R=60, n_b=60), "p10_k4_c500_r100": dict(k=4, P=10, C=500, R=100, n_b=120),
          "p10_k2_c50_r2000": dict(k=2, P=10, C=50, R=2000, n_b=400)}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, bubble, repeat, threshold, levels):
    samples, last = {}, None
    room = bubble.n_cands * bubble.n_paths ** bubble.ploidy
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        ov.phase_branch(bubble, False, 0, threshold, levels=levels, max_candidates=500, cap=room)
        wall = 1e3 * (time.perf_counter() - t0)
        last = ov.phase_stats()
        if i == 0:
            continue                                             # (one call outside the samples: the workspaces grow here)
        samples.setdefault("ms_wall", []).append(wall)
        for k, v in last.items():
            if k.startswith("ms_"):
                samples.setdefault(k, []).append(v)
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=11, help="calls per shape; medians, minima and maxima are reported")
    ap.add_argument("--only", default=None, help="one of the shapes")
    args = ap.parse_args(argv)
    import phase_utils as pu
    out = {"repeat": max(1, args.repeat)}
    ov = ExactOverlapper(device=0)
    for name, shape in SHAPES.items():
        if args.only and name != args.only:
            continue
        bubble = pu.bubble_of(pu.random_case(7, start=0, odd_reads=False, **shape))
        out[name] = {"default_threshold": measure(ov, bubble, args.repeat, 1e-3, None),
                     "keep_all": measure(ov, bubble, args.repeat, 0.0, None),
                     "keep_all_and_prune": measure(ov, bubble, args.repeat, 0.0, phasing.prune_levels(0.1, 0.1, 9))}
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
