#!/usr/bin/env python3
"""Developer probe: the config-2 read set through overlap -> layout stage 1 -> transitive reduction -> tip removal, once,
on the GPU, and from that one process the statistics of po_layout_tips (rounds included) beside the time of
po_layout_reduce on the same graph -- the yardstick DESIGN.md section 3.9c compares the tips against.

    python tools/tips_probe.py [--config cfg2] [--length-fuzz 1000] [--max-tip-length 4] [--max-tip-length-bases 5000] [--repeat 7]

The config-2 graph is clean (a handful of candidates, nothing to remove).  ``--tangle N`` runs a graph that is rich in tips
instead: the seeded ``tangle_case`` of tests/tips_utils.py with a line of N reads and N tips hung on it and on each other,
from GFA text, stage 1 -> tips (no reduction: the rows are the edges).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="cfg2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--length-fuzz", type=int, default=1000)
    ap.add_argument("--max-tip-length", type=int, default=4)
    ap.add_argument("--max-tip-length-bases", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=7, help="calls of stage 1, reduce and tips; medians, minima and maxima are reported")
    ap.add_argument("--tangle", type=int, default=0, help="a tip-rich synthetic graph of this many line reads and tips instead of --config")
    args = ap.parse_args(argv)
    if args.tangle:
        return tangle(args)
    ov = ExactOverlapper(device=0)
    for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
        ov.add_sequence(name, seq)
    rows = ov.overlaps_result(args.min_length)
    out = {"config": args.config, "repeat": max(1, args.repeat)}
    samples = {}

    def note(name, stats):
        out[name] = stats                                        # the last call's record; times of every call below
        for k, v in stats.items():
            if k.startswith("ms_"):
                samples.setdefault(name, {}).setdefault(k, []).append(v)

    for _ in range(out["repeat"]):
        edges, _ = ov.layout_edges(rows, want_removed=False)
        note("layout", ov.layout_stats())
        note("node_order", ov.node_order_stats())               # the two passes po_layout_edges runs for the tips
        kept = ov.layout_reduce(edges, args.length_fuzz)
        note("reduce", ov.reduce_stats())
        tipped = ov.layout_tips(kept, args.max_tip_length, args.max_tip_length_bases)
        note("tips", ov.tips_stats())
        again = ov.layout_tips(tipped, args.max_tip_length)      # the second application of assembler.py:177-179
        note("tips_again", ov.tips_stats())
        for r in (again, tipped, kept, edges):
            r.free()
    rows.free()
    ov.close()
    out["ms"] = {name: {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                        for k, v in d.items()} for name, d in samples.items()}
    med = lambda name: out["ms"][name]["ms_total"]["median"]   # noqa: E731
    out["tips_ms_over_reduce_ms"] = round(med("tips") / med("reduce"), 4) if med("reduce") else None
    out["node_order_ms_over_layout_ms"] = round(med("node_order") / med("layout"), 4) if med("layout") else None
    print(json.dumps(out))
    return 0


def tangle(args) -> int:
    import statistics as st
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import reduce_utils as ru
    import tips_utils as tu
    text = ru.gfa_text(*tu.tangle_case(1, n_line=args.tangle, n_tips=args.tangle))
    with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
        f.write(text)
        f.flush()
        ov = ExactOverlapper(device=0)
        _, rows = ov.add_gfa(f.name)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    rows.free()
    ms, stats = [], None
    for _ in range(max(1, args.repeat)):
        kept = ov.layout_tips(edges, args.max_tip_length, args.max_tip_length_bases)
        stats = ov.tips_stats()
        ms.append(stats["ms_total"])
        kept.free()
    edges.free()
    ov.close()
    print(json.dumps({"tangle": args.tangle, "repeat": len(ms), "tips": stats,
                      "ms_total": {"median": round(st.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
