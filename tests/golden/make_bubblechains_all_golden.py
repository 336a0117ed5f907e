#!/usr/bin/env python3
"""Generate tests/golden/bubblechain_all_cases.npz: the contract of po_layout_bubblechains_all and po_layout_contigs_all
 on every application, held against the reference's own functions, EXECUTED.

Runs only where the reference checkout is present (make_contigs_golden sets its path up); the output is committed.

    phasm.assembly_graph.build_bubblechains(component, 1)                        phasm/assembly_graph.py:594-652
    phasm.assembly_graph.identify_contigs(g, exclude_nodes, min_contig_len)      phasm/assembly_graph.py:655-718

Both run UNMODIFIED on the stand-in graph of make_contigs_golden.  build_bubblechains runs on every weakly connected
component of every application, with the one name it looks up in its module, ``find_superbubbles``, bound to the contract's
top-level pairs of that component (tests/cyclic_utils.py, held equal to the brute-forced definition by make_cyclic_golden).
That replacement is needed because the reference's own find_superbubbles cannot run here on a component with a cycle: its
graph_to_dag fails under the installed networkx at ``dfs_tree(...).nodes_iter`` and picks its root by ``random.choice``.
``superbubble_nodes``, the start tiers, the walk with its ``visited`` set and ``networkx.subgraph`` are the reference's.  It
runs with min_nodes 1 and is compared with the contract's chains before the filter: on a ring its chain is smaller than ours
(below), so the two filters need not agree; the filter itself is held by ``definition == scheme``.

  text cases    every text case of superbubble_all_cases.npz at (b) after the cleaning chain and (c) after
                merge_unambiguous_paths, with the edge weights and node lengths tests/test_contigs_oracle.py rebuilds
  direct cases  tests/bubblechain_all_utils.py direct_inputs(): those of cyclic_utils, then the rings this stage is about

Asserted on EVERY application:
    the ring-aware restated walk (``definition``) equals the scheme (``scheme``) in every array and count;
    where no bubble lies in an SCC, both equal bubblechain_utils.definition on the bubbles of the acyclic partitions;
    every chain of ours that is no ring is a chain of the reference, equal as (node set, edge count), and the reference
    yields no other chain outside the ring components; per ring the reference yields ONE chain, a subset of ours, and the
    difference is the strict interior of one top-level bubble of that ring (possibly empty): its walk starts at an entrance
    picked by the iteration order of a Python set and stops one bubble short, both ends of the closing bubble being visited;
    the reference's identify_contigs, given OUR exclude set (the nodes that carry a chain after the min_nodes filter), yields
    our contigs as sorted node tuples, for min_contig_len 5000 and 0.
And over all: at least 20 applications have a ring chain, and every situation of ``SITUATIONS`` occurs.

    --time    also print what the reference's build_bubblechains takes on the graphs tools/ringchains_probe.py measures, on
              this host core (best of 5 runs, find_superbubbles' replacement not included)"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_contigs_golden as mcg  # noqa: E402  (sets the paths up, installs the stand-in graph, raises the recursion limit)
import numpy as np  # noqa: E402
import phasm.assembly_graph as ag  # noqa: E402  (reference)

import bubblechain_all_utils as ba  # noqa: E402
import bubblechain_utils as bu  # noqa: E402
import components_utils as cu  # noqa: E402
import contig_utils as ct  # noqa: E402
import cyclic_utils as cy  # noqa: E402
import superbubble_utils as su  # noqa: E402
from test_contigs_oracle import stage_inputs as contig_stage_inputs  # noqa: E402

TIME = "--time" in sys.argv
SITUATIONS = ("ring_and_path_in_one_graph", "ring_with_nested_bubble", "ring_dropped_by_min_nodes", "power_of_two_ring",
              "ring_whose_leader_is_not_rank_0", "reference_one_bubble_short", "singleton_part_compared")
TIMED = ("direct_ring_1025_ascending", "direct_cy_four_node_digraphs_4096", "direct_cy_strong_union_2000", "cfg2_1k")


def node_length(n):
    """The length of node n of a direct case: what tests/test_gpu_components.py segments() gives its segment."""
    return 1000 + (n >> 1) % 97


def component_graphs(order, edges3, lengths, weak):
    """One stand-in graph per weakly connected component, nodes and edges in the graph's order (node names: id + 1)."""
    mcg.LNode.lengths = {n + 1: x for n, x in lengths.items()}
    graphs = [mcg.ContigGraph() for _ in range(weak["stats"]["n_components"])]
    comp_of = dict(zip(order, weak["node_component"].tolist()))
    for n in order:
        graphs[comp_of[n]].add_node(mcg.LNode(n + 1))
    for u, v, w in edges3:
        graphs[comp_of[u]].add_edge(mcg.LNode(u + 1), mcg.LNode(v + 1), weight=w, overlap_len=17)
    return graphs, comp_of


def reference_chains(graphs, comp_of, pairs, seconds=None):
    """build_bubblechains(component, 1) on every component -> per component the sorted (sorted node ids, edges) it yields."""
    mine = [[] for _ in graphs]
    for s, t in pairs:
        mine[comp_of[s]].append((mcg.LNode(s + 1), mcg.LNode(t + 1)))
    out = []
    for g, top in zip(graphs, mine):
        ag.find_superbubbles = lambda graph, report_nested=False, top=top: iter(top)
        t0 = time.perf_counter()
        found = list(ag.build_bubblechains(g, 1))
        if seconds is not None:
            seconds.append(time.perf_counter() - t0)
        out.append(sorted((sorted(int(n) - 1 for n in chain), chain.number_of_edges()) for chain in found))
    return out


def contig_record(res, edges4):
    """ct.record_of with the arrays as a digest above CONTIG_DIGEST_ABOVE edges: the file has to stay small, and the arrays of
    a larger case are still held in full by the restatement on the test's side."""
    rec = ct.record_of(res, edges4)
    if "sha256" not in rec and rec["n_edges"] > ba.CONTIG_DIGEST_ABOVE:
        rec = {k: v for k, v in rec.items() if not k.startswith("a_")}
        rec["sha256"] = cu.digest(*ct._canonical(res, edges4))
    return rec


def application(edges4, order, lengths, totals, extra, min_nodes=1, timed=None):
    order = [int(x) for x in order]
    edges4 = np.asarray(edges4, np.int64).reshape(-1, 4)
    uv = edges4[:, :2]
    sb = cy.scheme_all(uv.tolist(), order)
    plain, sync = ba.definition(uv, order, min_nodes, sb), ba.scheme(uv, order, min_nodes)
    for k in ba.ARRAY_KEYS:
        assert np.array_equal(plain[k], sync[k]), "the scheme differs from the definition: " + k
    assert {k: plain["stats"][k] for k in ba.STAT_KEYS} == {k: sync["stats"][k] for k in ba.STAT_KEYS}
    st = sync["stats"]
    assert st["n_ring_rounds"] == (ba.ring_rounds(st["n_top"]) if st["n_top"] and st["n_cyclic_bubbles"] else 0)
    if not st["n_cyclic_bubbles"]:                # no bubble in an SCC: the chains of the acyclic partitions
        old = bu.definition(uv, order, min_nodes, su.scheme(uv, order))
        for k in ba.ARRAY_KEYS:
            assert np.array_equal(old[k], sync[k]), "the singleton part differs from po_layout_bubblechains: " + k
        assert st["n_ring_chains"] == 0
        totals["singleton_part_compared"] += 1
    # the reference's build_bubblechains per weak component, against our chains before the filter
    weak = cu.weak_components(uv, order)
    graphs, comp_of = component_graphs(order, edges4[:, :3].tolist(), lengths, weak)
    top = [(int(s), int(t)) for s, t, nested in zip(sb["b_entrance"].tolist(), sb["b_exit"].tolist(), sb["b_nested"].tolist()) if not nested]
    sets = {int(s): set(x) for s, x in zip(sb["b_entrance"].tolist(), su.node_sets(sb, order))}
    ref = reference_chains(graphs, comp_of, top)
    every = plain if min_nodes == 1 else ba.definition(uv, order, 1, sb)
    exit_of = dict(top)
    ours = [[] for _ in graphs]
    for j in range(len(every["c_first"])):
        ours[comp_of[int(every["c_first"][j])]].append(j)
    short = 0
    for c, js in enumerate(ours):
        rings = [j for j in js if ba.is_ring(every, j)]
        if rings:
            assert len(js) == 1 and len(ref[c]) == 1, "a ring chain is a whole weakly connected component"
            j = rings[0]
            mine, (theirs, _) = set(bu.nodes_of(every, order, j)), ref[c][0]
            assert set(theirs) <= mine
            interiors, s = [], int(every["c_first"][j])
            for _ in range(int(every["c_bubbles"][j])):
                interiors.append(sets[s] - {s, exit_of[s]})
                s = exit_of[s]
            assert s == int(every["c_first"][j]) and mine - set(theirs) in interiors, "the reference is not one bubble short"
            short += bool(mine - set(theirs))
        else:
            want = sorted((sorted(bu.nodes_of(every, order, j)), int(every["c_edges"][j])) for j in js)
            assert want == ref[c], "the definition differs from the reference on a component without a ring"
    # the reference's identify_contigs on the whole graph with OUR exclude set
    X = sorted(int(n) for n, c in zip(order, sync["node_chain"].tolist()) if c != ba.NONE)
    whole = mcg.direct_graph(order, edges4[:, :3].tolist(), lengths)
    idx = lambda n: int(n) - 1   # noqa: E731
    contigs = []
    for min_len in (5000, 0):
        c_plain, c_sync = ct.definition(edges4, order, lengths, X, min_len), ct.scheme(edges4, order, lengths, X, min_len)
        for k in ct.ARRAY_KEYS:
            assert np.array_equal(c_plain[k], c_sync[k]), "contigs: the scheme differs from the definition: " + k
        ref_paths = mcg.reference(whole, idx, set(X), min_len)
        assert sorted(ct.paths_of(c_plain, edges4)) == ref_paths, "the contigs differ from the reference's"
        crec = contig_record(c_sync, edges4)
        crec["min_contig_len"] = min_len
        contigs.append(crec)
    rec = ba.record_of(sync, edges4)
    by = np.lexsort((uv[:, 1], uv[:, 0])) if len(uv) else np.zeros(0, np.int64)
    rec["in_sha256"] = cu.digest(order, uv[by], edges4[by, 2], [lengths[n] for n in order])
    rec.update(extra)
    rec["min_nodes"] = min_nodes
    rec.update({k: int(st[k]) for k in ba.SCHEME_KEYS})
    rec["contigs"] = contigs
    rec["ref_short_rings"] = short
    ring_js = [j for j in range(len(sync["c_first"])) if ba.is_ring(sync, j)]
    rank = {n: r for r, n in enumerate(order)}
    nested = set(sb["b_entrance"][sb["b_nested"] != 0].tolist())
    totals["applications"] += 1
    totals["with_a_ring_chain"] += st["n_ring_chains"] > 0
    totals["ring_chains"] += st["n_ring_chains"]
    totals["longest_ring"] = max([totals["longest_ring"]] + [int(sync["c_bubbles"][j]) for j in ring_js])
    totals["ring_and_path_in_one_graph"] += bool(ring_js) and len(ring_js) < st["n_chains"]
    totals["ring_with_nested_bubble"] += any(set(bu.nodes_of(sync, order, j)) & nested for j in ring_js)
    totals["ring_dropped_by_min_nodes"] += st["n_ring_chains"] > len(ring_js)
    totals["power_of_two_ring"] += any(int(sync["c_bubbles"][j]) & (int(sync["c_bubbles"][j]) - 1) == 0 for j in ring_js)
    totals["ring_whose_leader_is_not_rank_0"] += any(rank[int(sync["c_first"][j])] != 0 for j in ring_js)
    totals["reference_one_bubble_short"] += short > 0
    totals["digest_records"] += "sha256" in rec
    if timed:
        runs = []
        for _ in range(5):
            seconds = []
            reference_chains(graphs, comp_of, top, seconds)
            runs.append(sum(seconds))
        print("    the reference's build_bubblechains on %s (%s): %.3f ms (best of 5)" % (timed, extra["stage"], 1e3 * min(runs)))
    return rec


def main():
    ag.AssemblyGraph = mcg.ContigGraph
    mcg.mbg.msg.rgfa.AssemblyGraph = mcg.ContigGraph
    keys = ("applications", "with_a_ring_chain", "ring_chains", "longest_ring", "digest_records") + SITUATIONS
    totals = {k: 0 for k in keys}
    contig_cases = {c["name"]: c for c in ct.load_golden()["cases"]}
    cases = []
    for c in cy.load_golden()["cases"]:
        if c.get("direct"):
            continue
        stages = contig_stage_inputs(contig_cases[c["name"]])
        out = {"name": c["name"], "results": []}
        for stage, old in zip(("b", "c"), c["results"]):
            edges4, order, n_ids, lengths = stages[stage]
            uv = cu.uv_of(edges4)
            assert cu.digest(order, uv[np.lexsort((uv[:, 1], uv[:, 0]))]) == old["in_sha256"], "not the graph of superbubble_all_cases.npz"
            out["results"].append(application(edges4, order, lengths, totals, {"stage": stage, "n_ids": n_ids},
                                              timed=c["name"] if TIME and c["name"].endswith(TIMED[-1]) else None))
        b, cc = out["results"]
        print("%-30s b: %5d nodes %4d chains (%d rings)  c: %5d / %4d (%d)" % (c["name"], b["n_nodes"], b["n_chains"], b["n_ring_chains"],
                                                                              cc["n_nodes"], cc["n_chains"], cc["n_ring_chains"]), flush=True)
        cases.append(out)
    print("the text cases alone:", totals, flush=True)
    for name, order, edges, n_ids, min_nodes in ba.direct_inputs():
        edges4 = np.asarray([(u, v, 100, 17) for u, v in edges], np.int64).reshape(-1, 4)
        lengths = {int(n): node_length(int(n)) for n in order}
        rec = application(edges4, order, lengths, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(list(order) + [-2]) + 2},
                          min_nodes, timed=name if TIME and "direct_" + name in TIMED else None)
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        print("%-58s nodes %5d  %4d top-level, %4d chains (%d short), %d rings of %d bubbles, %d election rounds, the reference short on %d" % (
            "direct_" + name, rec["n_nodes"], rec["n_top"], rec["n_chains"], rec["n_short"], rec["n_ring_chains"], rec["n_ring_bubbles"],
            rec["n_ring_rounds"], rec["ref_short_rings"]), flush=True)
    for k, v in totals.items():
        assert v > 0 or k == "digest_records", "situation %s never occurs" % k
    assert totals["with_a_ring_chain"] >= 20, totals
    ba.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", ba.GOLDEN_FILE, len(cases), "cases", os.path.getsize(ba.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
