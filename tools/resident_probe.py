#!/usr/bin/env python3
"""Developer probe: one TURN of the walk's loop -- the gather of a bubble and its step -- by the two routes, from one process on
the GPU: what DESIGN.md section 3.9w records.

    python tools/resident_probe.py [--repeat 11] [--shapes walk,limit,long]

``parent`` is the route through the host: ``relevant_reads`` with the loop's two Python sets (sorted, uploaded, marked), eight
arrays home, ``DeviceWalk.step`` (``walk_paths``, the merge with the walk's host map, the arrays up again).  ``resident`` is
``DeviceWalk.relevant`` + ``step_resident``.  Two walks on one handle are advanced in lock-step, one by each route, and every
step's (cand, ext, rl) compared byte for byte; at the last bubble the turn is timed on both as a PEEK (``advance = 0``), which
runs everything but the take-over and can be repeated.  ``wall`` is the whole turn from Python objects to numpy arrays;
``device`` the ``ms_total`` of the gather's stats plus that of the step's (the resident gather does not wait for its last
launches, so its figure ends where the lists are made); ``new_kernels`` the ``ms_resident`` of the step.

Shapes: ``walk`` -- the last bubble of the synthetic walk of tests/test_gpu_resident.py; ``limit`` -- the defaults' limit of
section 3.9s (ploidy 4, 10 paths, about 500 candidates, 39 bubbles deep, 960 block reads at the end); ``long`` -- a block of 250
small bubbles (two paths of two reads), where what the parent route pays per step in the size of the block shows.
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


def timed(repeat, call):
    wall, dev, new = [], [], []
    for _ in range(repeat):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        d, n = call.device()
        dev.append(d)
        new.append(n)
    return {"wall_ms": spread(wall), "device_ms": spread(dev), "new_kernels_ms": spread(new)}


class Turns:
    """Two walks on one handle, one per route, over ``bubbles`` (dicts with cur, preds, path_reads, and the arguments of the step)."""

    def __init__(self, ov, index, ploidy):
        self.ov, self.index = ov, index
        self.host, self.res = ov.phase_walk(ploidy), ov.phase_walk(ploidy)
        self.prev_graph, self.prev_aligning = set(), set()

    def parent(self, b, args, advance):
        start = self.host.start_of_block
        rel = phasing.relevant_reads(self.ov, self.index, b["cur"], sorted(self.prev_graph), sorted(self.prev_aligning), b["preds"], start,
                                     b["min_spanning_reads"])
        self._gather_ms = self.ov.relevant_stats()["ms_total"]
        return rel, self.host.step(rel, b["path_reads"], start, *args, advance=advance)

    def resident(self, b, args, advance):
        g = self.res.relevant(self.ov, self.index, b["cur"], b["preds"], self.res.start_of_block, b["min_spanning_reads"])
        self._gather_ms = self.ov.relevant_stats()["ms_total"]
        out = self.res.step_resident(g, b["path_reads"], self.res.start_of_block, *args, advance=advance)
        fell = g.fell_back
        g.close()
        return fell, out

    def device(self):
        st = self.ov.walk_stats()
        return self._gather_ms + st["ms_total"], st["ms_resident"]

    def advance(self, b, args):
        rel, want = self.parent(b, args, True)
        fell, got = self.resident(b, args, True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)), "the two routes differ"
        if len(want[2]):
            self.prev_graph |= set(b["cur"])
            self.prev_aligning |= set(rel.cur_aligning.tolist())
        return rel, want

    def new_block(self):
        self.host.reset()
        self.res.reset()
        self.prev_graph, self.prev_aligning = set(), set()

    def measure(self, b, args, repeat):
        rel, want = self.parent(b, args, False)
        _, got = self.resident(b, args, False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)), "the two routes differ"
        info = self.res.info()
        assert info == self.host.info()
        out = {"shape": dict(info, n_paths=len(b["path_reads"]), n_relevant=len(rel.rel_reads), n_alignments=len(rel.aln_b), n_b=len(rel.b_reads),
                             n_prev_graph=len(self.prev_graph), n_prev_aligning=len(self.prev_aligning), n_final=len(want[2]))}
        for name, route in (("parent", self.parent), ("resident", self.resident)):
            call = lambda route=route: route(b, args, False)   # noqa: E731
            call.device = self.device
            timed(2, call)                                        # (warm: buffers of both routes at their size)
            out[name] = timed(repeat, call)
        return out

    def close(self):
        self.host.close()
        self.res.close()


def synthetic_walk(repeat):
    import resident_utils as rsu
    import walk_product_utils as wp
    walk = rsu.long_walk()
    p = walk["params"]
    ov = rsu.handle_for(walk)
    index = rsu.indexed(ov, walk)
    t = Turns(ov, index, 2)
    expand = wp.reads_of_node(walk)
    levels = phasing.prune_levels(0.29, p["prune_step_size"], p["max_prune_rounds"])
    last = max(j for j, s in enumerate(walk["trace"]) if s["arm"] == "advanced" and not s["broke"] and s["n_b"] > 256)
    out = None
    for j, s in enumerate(walk["trace"]):
        raw = walk["bubbles"][s["bubble"]]
        b = {"cur": raw["interior_reads"], "preds": raw["preds"], "min_spanning_reads": p["min_spanning_reads"],
             "path_reads": [[r for x in path[1:-1] for r in expand(x)] for path in raw["paths"]]}
        if s["broke"] or s["arm"] == "retry":
            t.new_block()
            if s["arm"] == "retry":
                continue
        args = (1e-3 if len(s["rel_reads"]) >= 5 else 0.5, p["min_spanning_reads"], levels, p["max_candidates"])
        if j == last:
            out = t.measure(b, args, repeat)
            break
        t.advance(b, args)
    t.close()
    index.free()
    ov.close()
    return out


def chain_shape(repeat, n_bubbles, per_bubble, P, k, R, C, threshold=0.0, seed=5):
    """A chain of ``n_bubbles`` bubbles of ``per_bubble`` new graph reads each, spread over ``P`` paths, and ``R`` reads outside
    the graph that each align to one read of every bubble (so every one of them spans every bubble).  Threshold 0 keeps every
    extension; the one prune level is chosen by a dry run so that about ``C`` candidates survive."""
    import relevant_utils as ru
    rng = np.random.default_rng(seed)
    n_graph = n_bubbles * per_bubble
    ov = ExactOverlapper()
    ru.add_reads(ov, [60000] * ((n_graph + R + 1) // 2))
    rows = []
    for d in range(n_bubbles):
        for r in range(R):
            a0 = int(rng.integers(0, 2000)) + 40 * d
            rows.append((n_graph + r, d * per_bubble + int(rng.integers(0, per_bubble)), a0, a0 + int(rng.integers(50, 1500)), 0, 100))
    res = ov.result_from_rows(ru.rows_array(rows))
    index = ov.phase_index(res)
    res.free()
    t = Turns(ov, index, k)
    out = None
    for d in range(n_bubbles):
        new = list(range(d * per_bubble, (d + 1) * per_bubble))
        b = {"cur": new, "preds": [], "min_spanning_reads": 0, "path_reads": [[x for j, x in enumerate(new) if j % P == q] for q in range(P)]}
        _, (_, _, rl) = t.parent(b, (threshold, 0, None, 0), False)
        level = float(np.sort(rl)[-min(C, len(rl))] - rl.max()) if len(rl) else 0.0
        args = (threshold, 0, [min(level, 0.0)], C)
        if d == n_bubbles - 1:
            out = t.measure(b, args, repeat)
            break
        t.advance(b, args)
    t.close()
    index.free()
    ov.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=11)
    ap.add_argument("--shapes", default="walk,limit,long")
    a = ap.parse_args()
    shapes = a.shapes.split(",")
    result = {}
    if "walk" in shapes:
        result["synthetic_walk"] = synthetic_walk(a.repeat)
    if "limit" in shapes:
        result["defaults_at_their_limit"] = chain_shape(a.repeat, n_bubbles=40, per_bubble=24, P=10, k=4, R=100, C=500)
    if "long" in shapes:
        result["long_block_small_bubble"] = chain_shape(a.repeat, n_bubbles=250, per_bubble=4, P=2, k=2, R=30, C=20)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
