#!/usr/bin/env python3
"""Generate tests/golden/paths_cases.npz by EXECUTING the reference's own functions and networkx.

Runs only where the reference checkout is present; the output (inputs and recorded results only) is committed.

    phasm.bubbles.find_superbubbles(g, report_nested=False)      phasm/bubbles.py:384-445
    phasm.bubbles.superbubble_nodes(g, s, t)                      phasm/bubbles.py:448-463
    networkx.all_simple_paths(g, s, t)                            as BubbleChainPhaser.phase() calls it, phasm/phasing.py:207-210
    g.predecessors_iter(t) with g[p][t]['weight']                 phasing.py:396

run unmodified on the stand-in graph of make_walk_golden.py (node names are id + 1: the finder tests the truth of a node).

Recorded per case: the inputs (node order, edges with weights in edge order, max_paths) and the result of the contract
 as tests/paths_utils.py ``definition`` states it.

Asserted below, before anything is written, on every case: ``definition`` equals the numpy ``scheme`` and ``HostPaths``; for every
bubble of ``definition`` the interior equals ``superbubble_nodes - {s, t}``, the predecessors equal ``predecessors_iter`` with
their weights in that order, and -- where the bubble is listed -- the paths equal ``networkx.all_simple_paths``, path for path
and in that order; on every case whose graph has no cycle and no self-loop the bubbles equal
``find_superbubbles(g, report_nested=False)`` as a set (cyclic partitions go through graph_to_dag in the reference and stay out of
the contract: those cases are pinned by the definition alone and counted); on every walk of walk_cases.npz the visiting order
and the recorded paths, interior_nodes and preds of every bubble equal the record."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.setrecursionlimit(20000)

import make_walk_golden as mwg  # noqa: E402  (sets the paths up and installs the stand-in graph; the reference is importable after it)
import networkx  # noqa: E402
import phasm.bubbles as rb  # noqa: E402  (reference)

import paths_utils as pp  # noqa: E402
import walk_utils as wu  # noqa: E402
from phasm_amd import phasing  # noqa: E402

assert rb.find_superbubbles.__code__.co_filename.startswith("/root/reference/")

WALK_MAX_PATHS = 1 << 20


def graph_of(order, edges):
    g = mwg.WalkGraph()
    for n in order:
        g.add_node(n + 1)
    for u, v, w in edges:
        g.add_edge(u + 1, v + 1, weight=w, overlap_len=mwg.NODE_OVERLAP)
    assert [n - 1 for n in g] == list(order)
    return g


def has_cycle(order, edges):
    indeg = {n: 0 for n in order}
    for _, v, _ in edges:
        indeg[v] += 1
    todo, seen = [n for n in order if indeg[n] == 0], 0
    succ = {n: [] for n in order}
    for u, v, _ in edges:
        succ[u].append(v)
    while todo:
        seen += 1
        for w in succ[todo.pop()]:
            indeg[w] -= 1
            if indeg[w] == 0:
                todo.append(w)
    return seen != len(order)


def application(name, order, edges, max_paths, totals):
    d = pp.definition(edges, order, max_paths)
    s = pp.scheme(edges, order, max_paths)
    pp.same(s, d)
    host = phasing.HostPaths(edges, order)
    pp.same(pp.result_of(host.phase_paths(None, max_paths), host.paths_stats()), d)
    g = graph_of(order, edges)
    acyclic = not has_cycle(order, edges)
    mine = list(zip(d["b_entrance"].tolist(), d["b_exit"].tolist()))
    if acyclic:
        found = sorted((a - 1, b - 1) for a, b in rb.find_superbubbles(g, report_nested=False))
        assert found == sorted(mine), "%s: the bubbles differ from find_superbubbles" % name
        totals["held_to_find_superbubbles"] += 1
    else:
        totals["pinned_by_the_definition_only"] += 1
    for b, (entrance, exit_) in enumerate(mine):
        inside = sorted(n - 1 for n in rb.superbubble_nodes(g, entrance + 1, exit_ + 1) - {entrance + 1, exit_ + 1})
        mine_inside = d["inside_nodes"][d["inside_off"][b]:d["inside_off"][b + 1]].tolist()
        assert sorted(mine_inside) == inside, "%s: interior of bubble %d" % (name, b)
        preds = [(p - 1, int(g[p][exit_ + 1]["weight"])) for p in g.predecessors_iter(exit_ + 1)]
        lo, hi = int(d["pred_off"][b]), int(d["pred_off"][b + 1])
        assert list(zip(d["pred_node"][lo:hi].tolist(), d["pred_weight"][lo:hi].tolist())) == preds, "%s: preds of bubble %d" % (name, b)
        if d["b_flags"][b] & pp.UNLISTED:
            totals["bubbles_unlisted"] += 1
            continue
        paths = [[n - 1 for n in p] for p in networkx.all_simple_paths(g, entrance + 1, exit_ + 1)]
        off = d["path_off"]
        listed = [d["path_nodes"][off[p]:off[p + 1]].tolist() for p in range(int(d["bubble_path_off"][b]), int(d["bubble_path_off"][b + 1]))]
        assert listed == paths, "%s: the paths of bubble %d differ from networkx.all_simple_paths" % (name, b)
        totals["bubbles_listed"] += 1
        totals["paths_compared"] += len(paths)
    rec = pp.record_of(s)
    totals["cases"] += 1
    return {"name": name, "order": [int(x) for x in order], "edges_flat": [int(x) for e in edges for x in e], "max_paths": int(max_paths),
            "acyclic": acyclic, "result": rec}, d


def main():
    totals = {k: 0 for k in ("cases", "held_to_find_superbubbles", "pinned_by_the_definition_only", "bubbles_listed", "bubbles_unlisted",
                             "paths_compared", "walks", "walk_bubbles")}
    cases = []
    for name, order, edges, max_paths in pp.direct_inputs():
        case, d = application("direct_" + name, order, edges, max_paths, totals)
        cases.append(case)
        print("%-52s %4d nodes %3d bubbles, paths %s" % (case["name"], len(order), len(d["b_entrance"]), case["result"]["b_paths"][:5]))
    for k, walk in enumerate(wu.load_golden()["walks"]):
        edges = [tuple(e) for e in wu.edges_of(walk)]
        order = pp.first_seen(edges)
        case, d = application("walk_" + walk["name"], order, edges, WALK_MAX_PATHS, totals)
        case["walk"] = k
        # the visiting order of phase() and what it computed per bubble
        bp = phasing.HostPaths(edges, order).phase_paths(None, WALK_MAX_PATHS)
        chains = sorted(set(bp.bubbles["chain"].tolist()))
        visited = [b for c in chains for b in bp.chain_bubbles(c)]
        assert len(chains) == 1 and [int(bp.bubbles["entrance"][b]) for b in visited] == [x["entrance"] for x in walk["bubbles"]]
        for b, want in zip(visited, walk["bubbles"]):
            assert int(bp.bubbles["exit"][b]) == want["exit"]
            assert [list(p) for p in bp.paths_of(b)] == want["paths"], "paths"
            assert bp.interior_of(b) == sorted(want["interior_nodes"], key=order.index), "interior_nodes"
            assert [list(p) for p in bp.preds_of(b)] == want["preds"], "preds"
            assert bp.is_large(b, walk["params"]["max_bubble_size"]) == (len(want["paths"]) > walk["params"]["max_bubble_size"])
        totals["walks"] += 1
        totals["walk_bubbles"] += len(visited)
        cases.append(case)
        print("%-52s %4d nodes %3d bubbles, %d visited" % (case["name"], len(order), len(d["b_entrance"]), len(visited)))
    assert totals["held_to_find_superbubbles"] >= 30 and totals["paths_compared"] >= 500 and totals["bubbles_unlisted"] >= 4, totals
    pp.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", pp.GOLDEN_FILE, len(cases), "cases", os.path.getsize(pp.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
