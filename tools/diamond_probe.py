#!/usr/bin/env python3
"""Developer probe: the config-2 read set through overlap -> layout stage 1 -> transitive reduction -> tip removal, once,
on the GPU, and from that one process the statistics of po_layout_diamonds (rounds included) over repeated calls on the
tipped graph beside those of po_layout_tips on the same graph -- the yardstick DESIGN.md section 3.9d compares the
diamonds against.

    python tools/diamond_probe.py [--config cfg2] [--length-fuzz 1000] [--max-tip-length 4] [--max-tip-length-bases 5000] [--repeat 21]

The config-2 graph is clean (next to no candidates, nothing to remove): the figure is launch and readback latency.
``--cases NAME...`` runs text cases of tests/golden/diamond_cases.npz instead (the hubs settle one end node per round):
from GFA text, stage 1 -> reduction -> tips -> diamonds, rounds and device times of the diamond call.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phasm_amd import synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(ov, tipped, args):
    """Alternating calls of diamonds and tips on one edge result: the last stats of each and the spread of every time."""
    samples, last = {}, {}
    for _ in range(max(1, args.repeat)):
        for name, call, stats in (("diamonds", lambda: ov.layout_diamonds(tipped), ov.diamond_stats),
                                  ("tips", lambda: ov.layout_tips(tipped, args.max_tip_length, args.max_tip_length_bases), ov.tips_stats)):
            call().free()
            last[name] = stats()
            for k, v in last[name].items():
                if k.startswith("ms_"):
                    samples.setdefault(name, {}).setdefault(k, []).append(v)
    ms = {name: {k: spread(v) for k, v in d.items()} for name, d in samples.items()}
    return last, ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="cfg2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--min-length", type=int, default=1000)
    ap.add_argument("--length-fuzz", type=int, default=1000)
    ap.add_argument("--max-tip-length", type=int, default=4)
    ap.add_argument("--max-tip-length-bases", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=21, help="calls of diamonds and of tips on the tipped graph; medians, minima and maxima are reported")
    ap.add_argument("--cases", nargs="*", default=None, help="text cases of tests/golden/diamond_cases.npz instead of --config")
    args = ap.parse_args(argv)
    if args.cases is not None:
        return golden_cases(args)
    ov = ExactOverlapper(device=0)
    for name, seq in synth.oriented(synth.generate_reads(synth.CONFIGS[args.config])):
        ov.add_sequence(name, seq)
    rows = ov.overlaps_result(args.min_length)
    edges, _ = ov.layout_edges(rows, want_removed=False)
    reduced = ov.layout_reduce(edges, args.length_fuzz)
    tipped = ov.layout_tips(reduced, args.max_tip_length, args.max_tip_length_bases)
    ov.layout_diamonds(tipped).free()                            # (one call outside the samples: the workspaces grow here)
    last, ms = measure(ov, tipped, args)
    out = {"config": args.config, "repeat": max(1, args.repeat), "n_edges": len(tipped), "diamonds": last["diamonds"], "tips": last["tips"], "ms": ms}
    med = lambda name: ms[name]["ms_total"]["median"]   # noqa: E731
    out["diamonds_ms_over_tips_ms"] = round(med("diamonds") / med("tips"), 4) if med("tips") else None
    for r in (tipped, reduced, edges, rows):
        r.free()
    ov.close()
    print(json.dumps(out))
    return 0


def golden_cases(args) -> int:
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import diamond_utils as du
    cases = {c["name"]: c for c in du.load_golden()["cases"] if not c.get("direct")}
    names = args.cases or [n for n in cases if n.startswith("reduced_hub_")]
    out = {"repeat": max(1, args.repeat), "cases": {}}
    for name in names:
        c = cases[name]
        with tempfile.NamedTemporaryFile("w", suffix=".gfa") as f:
            f.write(du.case_text(c))
            f.flush()
            ov = ExactOverlapper(device=0)
            _, rows = ov.add_gfa(f.name)
        edges, _ = ov.layout_edges(rows, **c["params"])
        rows.free()
        reduced = ov.layout_reduce(edges, args.length_fuzz)
        tipped = ov.layout_tips(reduced, args.max_tip_length, args.max_tip_length_bases)
        ov.layout_diamonds(tipped).free()
        last, ms = measure(ov, tipped, args)
        d = last["diamonds"]
        out["cases"][name] = {"n_edges": len(tipped), "n_candidates": d["n_candidates"], "n_diamonds": d["n_diamonds"], "n_rounds": d["n_rounds"],
                              "diamonds_ms_total": ms["diamonds"]["ms_total"], "diamonds_ms_rounds": ms["diamonds"]["ms_rounds"],
                              "tips_ms_total": ms["tips"]["ms_total"]}
        for r in (tipped, reduced, edges):
            r.free()
        ov.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
