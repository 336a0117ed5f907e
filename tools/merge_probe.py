#!/usr/bin/env python3
"""Developer probe: the config-2 read set through overlap -> layout stage 1 -> the four cleaning calls, once, on the GPU,
and from that one process the statistics of po_layout_merge (rounds and the ms_* of every phase) over repeated calls on
the cleaned graph beside the ms_total of the four cleaning calls in the same run -- what DESIGN.md section 3.9e records.

    python tools/merge_probe.py [--config cfg2] [--repeat 21]
    python tools/merge_probe.py --tangle N        the seeded tangle of tests/tips_utils.py on a line of N reads with N tips
    python tools/merge_probe.py --lasso N         a ring of N reads with a tail of 8 (tests/merge_utils.py): four paths, two of
                                                  N nodes -- the ranking at depth, ceil(log2(N)) + 1 rounds
    python tools/merge_probe.py --ring N          N reads tiled round a circle: two pure link cycles and no head, so no
                                                  round is launched -- the links, number and emit phases alone

The point of comparison is the reference's merge_unambiguous_paths on a host core: tests/golden/make_merge_golden.py --time.
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


def measure(ov, edges, args):
    """The chain and the merge, ``repeat`` times: the last stats of the merge, the spread of its times and of the chain's."""
    samples, last = {}, None
    for i in range(max(1, args.repeat) + 1):
        chain_ms = 0.0
        cur = edges
        for call, stats in ((lambda r: ov.layout_reduce(r, args.length_fuzz), ov.reduce_stats),
                            (lambda r: ov.layout_tips(r, args.max_tip_length, args.max_tip_length_bases), ov.tips_stats),
                            (ov.layout_diamonds, ov.diamond_stats),
                            (lambda r: ov.layout_tips(r, args.max_tip_length, 5000), ov.tips_stats)):
            nxt = call(cur)
            chain_ms += stats()["ms_total"]
            if cur is not edges:
                cur.free()
            cur = nxt
        merged = ov.layout_merge(cur)
        last = dict(ov.merge_stats(), n_edges_cleaned=len(cur))
        merged.free()
        cur.free()
        if i == 0:
            continue                                             # (one pass outside the samples: the workspaces grow here)
        samples.setdefault("clean_ms_total", []).append(chain_ms)
        for k, v in last.items():
            if k.startswith("ms_"):
                samples.setdefault(k, []).append(v)
    return last, {k: spread(v) for k, v in samples.items()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="cfg2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--length-fuzz", type=int, default=1000)
    ap.add_argument("--max-tip-length", type=int, default=4)
    ap.add_argument("--max-tip-length-bases", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=21, help="passes of the chain and the merge; medians, minima and maxima are reported")
    ap.add_argument("--tangle", type=int, default=None, metavar="N")
    ap.add_argument("--lasso", type=int, default=None, metavar="N")
    ap.add_argument("--ring", type=int, default=None, metavar="N")
    args = ap.parse_args(argv)
    ov = ExactOverlapper(device=0)
    if args.tangle is not None or args.ring is not None or args.lasso is not None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import merge_utils as mu
        import reduce_utils as ru
        import tips_utils as tu
        if args.ring is not None:
            what, case = "ring_%d" % args.ring, mu.ring_case(args.ring)
        elif args.lasso is not None:
            what, case = "lasso_%d" % args.lasso, mu.lasso_case(args.lasso)
        else:
            what, case = "tangle_%d" % args.tangle, tu.tangle_case(3, n_line=args.tangle, n_tips=args.tangle)
        with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
            f.write(ru.gfa_text(*case))
            f.flush()
            _, rows = ov.add_gfa(f.name)
    else:
        what = args.config
        for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
            ov.add_sequence(name, seq)
        rows = ov.overlaps_result(args.min_length)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    rows.free()
    last, ms = measure(ov, edges, args)
    out = {"graph": what, "repeat": max(1, args.repeat), "n_edges_stage1": len(edges), "merge": last, "ms": ms}
    med = lambda name: ms[name]["median"]   # noqa: E731
    out["merge_ms_over_clean_ms"] = round(med("ms_total") / med("clean_ms_total"), 4) if med("clean_ms_total") else None
    edges.free()
    ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
