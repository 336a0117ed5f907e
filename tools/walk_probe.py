#!/usr/bin/env python3
"""Developer probe: one bubble of a walk by the two routes, from one process on the GPU -- what DESIGN.md section 3.9s records.

    python tools/walk_probe.py [--repeat 11] [--limit]

``branch`` is the route without a resident walk: ``bubble_from_relevant`` rebuilds the read sets of every slot of every candidate
in Python, ``po_phase_branch`` uploads them and scores.  ``walk`` is ``po_walk_step`` on a ``DeviceWalk`` that holds those sets as
bit rows.  Both are timed on the SAME bubble: the LAST bubble of the longest block of a synthetic walk (the one
tests/test_gpu_walk_state.py uses: 27 bubbles of two paths, ploidy 2, up to 120 candidates, 264 block reads at the end), with the
state the walk has there.  The walk route is timed as a peek (``advance = 0``), which runs everything but ``k_wk_advance`` and
leaves the state as it is, so it can be repeated; the cost of the advance itself is reported from ``po_get_walk_stats`` over the
walk's own steps.  ``wall`` is the whole call from Python objects to numpy arrays, ``device`` the ``ms_total`` of the stats.

``--limit`` adds a shape at the limits of the command's defaults: ploidy 4, 10 paths, 500 candidates, 40 bubbles deep, random
alignments; every step keeps all 5 000 000 extensions and prunes them to the 500 of greatest log_rl.
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

from phasm_amd import phasing  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(repeat, call, device_ms):
    wall, dev = [], []
    for _ in range(repeat):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(device_ms())
    return {"wall_ms": spread(wall), "device_ms": spread(dev)}


def synthetic(repeat):
    import relevant_utils as ru
    import test_gpu_walk_state as tw
    import walk_product_utils as wp
    import walk_utils as wu
    walk = tw.long_walk()
    p = walk["params"]
    ov = ExactOverlapper()
    ru.add_reads(ov, walk["lengths"])
    res = ov.result_from_rows(ru.rows_array(wu.rows_of(walk)))
    index = ov.phase_index(res)
    res.free()
    dw = ov.phase_walk(2)
    advance_ms, prev_graph, prev_aligning = [], set(), set()
    expand = wp.reads_of_node(walk)
    levels = phasing.prune_levels(0.29, p["prune_step_size"], p["max_prune_rounds"])
    last = max(j for j, s in enumerate(walk["trace"]) if s["arm"] == "advanced")
    out = {}
    for j, s in enumerate(walk["trace"]):
        b = walk["bubbles"][s["bubble"]]
        if s["arm"] != "advanced":
            raise SystemExit("the probe expects the walk of the test: every bubble advances, one new_block by too few spanning reads")
        start = dw.start_of_block
        rel = phasing.relevant_reads(ov, index, b["interior_reads"], sorted(prev_graph), sorted(prev_aligning), b["preds"], start, p["min_spanning_reads"])
        if rel.fell_back:
            dw.reset()
            prev_graph, prev_aligning, start = set(), set(), True
        path_reads = [[r for x in path[1:-1] for r in expand(x)] for path in b["paths"]]
        args = (path_reads, start, p["threshold"], p["min_spanning_reads"], levels, p["max_candidates"])
        if j == last:
            n = dw.info()["n_cands"]
            sets = dw.read_sets(range(n))
            out["shape"] = {"bubble": s["bubble"], "n_cands": n, "depth": dw.info()["depth"], "n_block_reads": dw.info()["n_block_reads"],
                            "n_relevant": len(rel.rel_reads), "n_b": len(rel.b_reads), "ids_in_the_sets": sum(len(x) for c in sets for x in c)}

            def by_branch():
                bubble = phasing.bubble_from_relevant(rel, 2, path_reads, sets)
                return ov.phase_branch(bubble, start, p["min_spanning_reads"], p["threshold"], levels=levels, max_candidates=p["max_candidates"])

            def pack_only():
                phasing.bubble_from_relevant(rel, 2, path_reads, sets)

            want, got = by_branch(), dw.step(rel, *args, advance=False)
            assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(want, got)), "the two routes differ"
            out["branch"] = timed(repeat, by_branch, lambda: ov.phase_stats()["ms_total"])
            out["pack_bubble_only"] = timed(repeat, pack_only, lambda: 0.0)["wall_ms"]
            out["walk"] = timed(repeat, lambda: dw.step(rel, *args, advance=False), lambda: ov.walk_stats()["ms_total"])
        dw.step(rel, *args)
        advance_ms.append(ov.walk_stats()["ms_advance"])
        prev_graph |= set(b["interior_reads"])
        prev_aligning |= set(rel.cur_aligning.tolist())
    out["advance_ms_over_the_walk"] = spread(advance_ms)
    dw.close()
    index.free()
    ov.close()
    return out


def limit(repeat, k=4, P=10, C=500, depth=40, R=100, per_bubble=24):
    """Random bubbles: ``per_bubble`` new graph reads each, spread over the paths; every relevant read aligns to a dozen of the
    block's reads.  Threshold 0 keeps every extension; one prune level far below keeps them all, max_candidates cannot cut (the
    reference's loop only raises the level), so the list is cut to C by taking ``cap`` -- the state takes the whole list, hence
    the levels are chosen so that about C survive: the level is the C-th greatest distance of a dry run."""
    rng = np.random.default_rng(5)
    ov = ExactOverlapper()
    dw = ov.phase_walk(k)
    out, step_ms, adv_ms = {}, [], []
    block = []
    for d in range(depth):
        new = list(range(d * per_bubble, (d + 1) * per_bubble))
        block += new
        b_reads = np.asarray(block, dtype=np.uint32)
        aln = [sorted(rng.choice(len(block), size=min(12, len(block)), replace=False).tolist()) for _ in range(R)]
        off = np.zeros(R + 1, np.uint32)
        off[1:] = np.cumsum([len(a) for a in aln])
        a0 = rng.integers(0, 2000, int(off[-1])).astype(np.int32)
        rel = phasing.RelevantReads(np.zeros(0, np.uint32), np.arange(R, dtype=np.uint32), np.full(R, 4000, np.int32), off,
                                    np.asarray([x for a in aln for x in a], np.uint32), a0, (a0 + rng.integers(50, 1500, len(a0))).astype(np.int32),
                                    b_reads)
        path_reads = [[new[j] for j in range(len(new)) if j % P == q] for q in range(P)]
        start = dw.start_of_block
        _, _, rl = dw.step(rel, path_reads, start, 0.0, 0, levels=None, advance=False)
        level = float(np.sort(rl)[-min(C, len(rl))] - rl.max()) if len(rl) else 0.0
        args = (path_reads, start, 0.0, 0, [min(level, 0.0)], C)
        if d == depth - 1:
            out["shape"] = dict(dw.info(), n_paths=P, n_relevant=R, n_b=len(block), n_extensions=dw.info()["n_cands"] * P ** k)
            n = dw.info()["n_cands"]
            sets = dw.read_sets(range(n))

            def by_branch():
                bubble = phasing.bubble_from_relevant(rel, k, path_reads, sets)
                return ov.phase_branch(bubble, start, 0, 0.0, levels=args[4], max_candidates=C)

            want, got = by_branch(), dw.step(rel, *args, advance=False)
            assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(want, got)), "the two routes differ"
            out["branch"] = timed(repeat, by_branch, lambda: ov.phase_stats()["ms_total"])
            out["pack_bubble_only"] = timed(repeat, lambda: phasing.bubble_from_relevant(rel, k, path_reads, sets), lambda: 0.0)["wall_ms"]
            out["walk"] = timed(repeat, lambda: dw.step(rel, *args, advance=False), lambda: ov.walk_stats()["ms_total"])
        t = time.perf_counter()
        dw.step(rel, *args)
        step_ms.append((time.perf_counter() - t) * 1e3)
        adv_ms.append(ov.walk_stats()["ms_advance"])
    out["step_wall_ms_over_the_walk"], out["advance_ms_over_the_walk"] = spread(step_ms), spread(adv_ms)
    dw.close()
    ov.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=11)
    ap.add_argument("--limit", action="store_true")
    a = ap.parse_args()
    result = {"synthetic_walk": synthetic(a.repeat)}
    if a.limit:
        result["defaults_at_their_limit"] = limit(a.repeat)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
