#!/usr/bin/env python3
"""Developer probe: the statistics of po_phase_index and po_phase_relevant (keys, the largest segment, the ms_* of every step and
the wall time of the call) over repeated calls, from one process on the GPU -- what DESIGN.md section 3.9o records.

    python tools/relevant_probe.py [--repeat 21]
        index.cfg2_1k     the index of the 151 182 rows of tests/golden/cfg2_1k.npz
        index.union       the index of the union of tests/test_gpu_relevant.py: disjoint copies of the golden cases, 530 000+ rows
        gather.bubble     one small bubble (case "bubble", query 2) on the union's index
        gather.hub        the hub query (case "degrees", query 1: six hubs relevant, 1 240 b reads) on the union's index

The wall time of the index is the whole call on a row result that is on the device already; that of the gather is the whole call
from Python lists to numpy arrays.  The point of comparison is the reference's dict build and get_relevant_read_info on a host
core, which tests/golden/make_relevant_golden.py times (--timings for the two large builds).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def sample(call, stats, repeat):
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
    return {"stats": last, "spread": {k: spread(v) for k, v in samples.items()}}


def index_probe(ov, rows, repeat):
    import relevant_utils as ru
    res = ov.result_from_rows(ru.rows_array(rows))
    ov.phase_index(res).free()                                   # (the rows go to the device here)
    kept = []

    def call():
        for old in kept:
            old.free()
        kept[:] = [ov.phase_index(res)]
    out = sample(call, ov.phase_index_stats, repeat)
    res.free()
    return out, kept[0]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=21, help="calls per measurement; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    import relevant_utils as ru
    out = {"repeat": max(1, args.repeat)}
    with np.load(os.path.join(ROOT, "tests", "golden", "cfg2_1k.npz")) as z:
        rows, n_seg = z["rows"].astype(np.int64), int(z["n_oriented"]) // 2
    ov = ExactOverlapper(device=0)
    ru.add_reads(ov, [10000] * n_seg)
    out["index.cfg2_1k"], index = index_probe(ov, rows, args.repeat)
    index.free()
    ov.close()
    cases = ru.load_golden()["cases"]
    per_copy = sum(len(ru.rows_of(c)) for c in cases)
    lengths, rows, shifts = ru.union_case(cases, -(-530000 // per_copy))
    ov = ExactOverlapper(device=0)
    ru.add_reads(ov, lengths)
    out["index.union"], index = index_probe(ov, rows, args.repeat)
    middle = (len(shifts) // len(cases) // 2) * len(cases)
    for name, ci, qi in (("gather.bubble", 1, 2), ("gather.hub", 3, 1)):
        q = ru.shifted_query(cases[ci]["queries"][qi], shifts[middle + ci])
        out[name] = sample(lambda: ru.query_source(ov, index, q), ov.relevant_stats, args.repeat)
    index.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
