#!/usr/bin/env python3
"""Generate tests/golden/bubblechain_cases.npz by EXECUTING the reference's own function.

Runs only where the reference checkout is present (make_merge_golden sets its path up); the output is committed.

    phasm.assembly_graph.build_bubblechains(component, min_nodes)      phasm/assembly_graph.py:594-652

run unmodified, per weakly connected component, on the stand-in graph of make_superbubbles_golden (with the recursion limit
that module raises), on every component in which every strongly connected component is a singleton and no node has a
self-loop.  It calls the reference's find_superbubbles(g, report_nested=False), superbubble_nodes and networkx.subgraph.

Recorded per application: the result of the contract as tests/bubblechain_utils.py states it, and
from the reference the set of (node set, number of edges) of the chains it yields on the components it ran on.

  text cases   every text case of merge_cases.npz at (b) after the cleaning chain of assembler.py:145-182 and (c) after
               merge_unambiguous_paths -- the applications of superbubble_cases.npz, with min_nodes 1
  direct cases tests/bubblechain_utils.py direct_inputs(): those of superbubble_utils with min_nodes 1, then the shapes
               this stage is about, some with another min_nodes

Asserted below: the restated walk (``definition``) equals the device's scheme run synchronously (``scheme``) in every array
on every application; on every component that qualifies the set of (node set, edge count) the reference yields equals the
definition's; at least 100 applications are compared with the reference, at least 50 of them have a chain in a qualifying
component, at least 40 a chain of at least two bubbles, and the longest chain has at least 1 024.

    --time    also print what the reference's build_bubblechains takes on the paths of 1 025 nodes and on the cleaned (b)
              and merged (c) graph of cfg2_1k, on this host core (best of 5 runs)"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_superbubbles_golden as msg  # noqa: E402  (sets the paths up, installs the stand-in graph, raises the recursion limit)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.bubbles as rb  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import bubblechain_utils as bu  # noqa: E402
import components_utils as cu  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import superbubble_utils as su  # noqa: E402

TIME = "--time" in sys.argv


class BubblechainGraph(msg.SuperbubbleGraph):
    def subgraph(self, nbunch):
        h = BubblechainGraph(**self.graph)
        nbunch = set(nbunch)
        for n in self.adj:                  # (node order kept)
            if n in nbunch:
                h.add_node(n)
        for u in h.adj:
            for v, d in self.adj[u].items():
                if v in h.adj:
                    h.add_edge(u, v, d)
        return h

    def in_degree(self, n):
        return len(self.pred[n])

    def out_degree(self, n):
        return len(self.adj[n])


def qualifies(component):
    """Every strongly connected component a singleton and no self-loop: the acyclic partition is the whole component."""
    if any(component.has_edge(n, n) for n in component):
        return False
    parts = list(rb.partition_graph(component))
    return len(parts) == 1 and parts[0][1]


def reference(g, idx, weak, min_nodes, seconds=None):
    """The reference on every component of g that qualifies -> (component numbers, sorted (sorted node ids, edges) per chain)."""
    nodes_of = [[] for _ in range(weak["stats"]["n_components"])]
    for n, c in zip(g, weak["node_component"].tolist()):
        nodes_of[c].append(n)
    compared, chains = [], []
    for c, nodes in enumerate(nodes_of):
        component = g.subgraph(nodes)
        if not qualifies(component):
            continue
        t0 = time.perf_counter()
        found = list(ag.build_bubblechains(component, min_nodes))
        if seconds is not None:
            seconds.append(time.perf_counter() - t0)
        compared.append(c)
        for chain in found:
            chains.append((sorted(idx(n) for n in chain), chain.number_of_edges()))
    return compared, sorted(chains)


def chains_of(res, order, comp_of, compared):
    """The same shape from a ``definition``-shaped result, on the components ``compared``."""
    on, out = set(compared), []
    for j, (first, k) in enumerate(zip(res["c_first"].tolist(), res["c_edges"].tolist())):
        if comp_of[first] in on:
            out.append((sorted(bu.nodes_of(res, order, j)), k))
    return sorted(out)


def application(g, idx, totals, extra, min_nodes=1, seconds=None):
    order = [idx(n) for n in g]
    edges = mdg.edge_array(g, idx)
    weak = cu.weak_components(edges, order)
    sb = su.scheme(edges, order)
    plain = bu.definition(edges, order, min_nodes, sb)
    sync = bu.scheme(edges, order, min_nodes, sb)
    for k in bu.ARRAY_KEYS:
        assert np.array_equal(plain[k], sync[k]), "the scheme differs from the definition: " + k
    assert {k: plain["stats"][k] for k in bu.STAT_KEYS} == {k: sync["stats"][k] for k in bu.STAT_KEYS}
    nest_bound, chain_bound = bu.round_bounds(sync["stats"])
    assert sync["stats"]["n_nest_rounds"] <= nest_bound and sync["stats"]["n_chain_rounds"] <= chain_bound
    compared, ref_chains = reference(g, idx, weak, min_nodes, seconds)
    comp_of = dict(zip(order, weak["node_component"].tolist()))
    mine = chains_of(plain, order, comp_of, compared)
    assert mine == ref_chains, "the definition differs from the reference"
    rec = bu.record_of(sync, edges)
    e = cu.uv_of(edges)
    rec["in_sha256"] = cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))])
    rec.update(extra)
    rec["min_nodes"] = min_nodes
    rec.update({k: sync["stats"][k] for k in bu.SCHEME_KEYS})
    rec["ref_components"] = compared
    if rec["n_edges"] > bu.DIGEST_ABOVE:
        rec["ref_sha256"] = cu.digest([k for _, k in ref_chains], [len(x) for x, _ in ref_chains], [n for x, _ in ref_chains for n in x])
    else:
        rec["ref_chain_edges"] = [k for _, k in ref_chains]
        rec["ref_chain_sizes"] = [len(x) for x, _ in ref_chains]
        rec["ref_chain_nodes"] = [n for x, _ in ref_chains for n in x]
    st = sync["stats"]
    on = set(compared)
    qualifying = [int(b) for f, b in zip(sync["c_first"].tolist(), sync["c_bubbles"].tolist()) if comp_of[f] in on]
    totals["applications"] += 1
    totals["compared_with_the_reference"] += bool(compared)
    totals["with_a_chain_in_a_qualifying_component"] += bool(ref_chains)
    totals["with_a_chain_of_at_least_2_bubbles"] += any(b >= 2 for b in qualifying)
    totals["longest_chain"] = max([totals["longest_chain"]] + qualifying)
    totals["reference_chains"] += len(ref_chains)
    totals["components_not_qualifying"] += weak["stats"]["n_components"] - len(compared)
    totals["nested_bubbles"] += st["n_bubbles"] - st["n_top"]
    totals["short_chains"] += st["n_short"]
    totals["several_chains_in_one_component"] += len({comp_of[f] for f in sync["c_first"].tolist()}) < st["n_chains"]
    totals["max_nest_rounds"] = max(totals["max_nest_rounds"], st["n_nest_rounds"])
    totals["max_chain_rounds"] = max(totals["max_chain_rounds"], st["n_chain_rounds"])
    totals["digest_records"] += "sha256" in rec
    return rec


def best_of_5(g, idx, min_nodes=1):
    order = [idx(n) for n in g]
    weak = cu.weak_components(mdg.edge_array(g, idx), order)
    runs = []
    for _ in range(5):
        seconds = []
        reference(g, idx, weak, min_nodes, seconds)
        runs.append(sum(seconds))
    return min(runs)


def text_case(c, totals):
    name, params = c["name"], c["params"]
    text = mu.case_text(c)
    out = {"name": name, "results": []}
    g, node_index = mrg.stage1_graph(text, params)
    idx0 = lambda n: node_index[str(n)]   # noqa: E731
    n_ids = len(node_index)
    g.remove_edges_from(ag.remove_transitive_edges(g, du.STAGE_FUZZ))
    ag.make_symmetric(g)
    ag.remove_tips(g, du.STAGE_L, du.STAGE_B)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    ag.remove_diamond_tips(g)
    ag.remove_tips(g, du.STAGE_L)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    timed = TIME and name.endswith("cfg2_1k")
    out["results"].append(application(g, idx0, totals, {"stage": "b", "n_ids": n_ids}))
    sec_b = best_of_5(g, idx0) if timed else 0.0
    ag.merge_unambiguous_paths(g)
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}
    idx = lambda n: n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)   # noqa: E731
    out["results"].append(application(g, idx, totals, {"stage": "c", "n_ids": n_ids}))
    b, cc = out["results"]
    line = "%-30s b: %5d nodes %4d chains (longest %d)  c: %5d / %4d (%d)" % (
        name, b["n_nodes"], b["n_chains"], b["max_chain_bubbles"], cc["n_nodes"], cc["n_chains"], cc["max_chain_bubbles"])
    if timed:
        line += "  the reference's build_bubblechains: (b) %.3f ms, (c) %.3f ms (best of 5)" % (1e3 * sec_b, 1e3 * best_of_5(g, idx))
    print(line)
    return out


def direct_graph(order, edges):
    """The direct case under truthy node names: node id + 1."""
    g = BubblechainGraph()
    for n in order:
        g.add_node(n + 1)
    for u, v in edges:
        g.add_edge(u + 1, v + 1, weight=100, overlap_len=17)
    return g


def main():
    ag.AssemblyGraph = BubblechainGraph
    msg.rgfa.AssemblyGraph = BubblechainGraph
    keys = ("applications", "compared_with_the_reference", "with_a_chain_in_a_qualifying_component", "with_a_chain_of_at_least_2_bubbles",
            "longest_chain", "reference_chains", "components_not_qualifying", "nested_bubbles", "short_chains",
            "several_chains_in_one_component", "max_nest_rounds", "max_chain_rounds", "digest_records")
    totals = {k: 0 for k in keys}
    idx = lambda n: n - 1   # noqa: E731
    cases = []
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
    reused = len(su.direct_inputs())
    for i, (name, order, edges, n_ids, min_nodes) in enumerate(bu.direct_inputs()):
        if i == reused:
            print("the reused applications alone:", {k: totals[k] for k in keys[:5]})
            assert (totals["applications"], totals["compared_with_the_reference"], totals["with_a_chain_in_a_qualifying_component"],
                    totals["with_a_chain_of_at_least_2_bubbles"], totals["longest_chain"]) == (301, 125, 71, 59, 1024), totals
        g = direct_graph(order, edges)
        assert [idx(n) for n in g] == list(order) and sorted((idx(u), idx(v)) for u, v in g.edges_iter()) == sorted(edges)
        rec = application(g, idx, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(list(order) + [-2]) + 2}, min_nodes)
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        line = "%-58s nodes %5d  %4d top-level, %4d chains (%d short, longest %d), rounds %d + %d" % (
            "direct_" + name, rec["n_nodes"], rec["n_top"], rec["n_chains"], rec["n_short"], rec["max_chain_bubbles"], rec["n_nest_rounds"],
            rec["n_chain_rounds"])
        if TIME and name.startswith("sb_path_1025"):
            line += "  the reference's build_bubblechains: %.3f ms (best of 5)" % (1e3 * best_of_5(g, idx))
        print(line)
    for k, v in totals.items():
        assert v > 0 or k == "digest_records", "situation %s never occurs" % k
    assert totals["compared_with_the_reference"] >= 100 and totals["with_a_chain_in_a_qualifying_component"] >= 50, totals
    assert totals["with_a_chain_of_at_least_2_bubbles"] >= 40 and totals["longest_chain"] >= 1024, totals
    assert totals["max_nest_rounds"] > 8 and totals["max_chain_rounds"] > 8, totals       # both loops cross a batch
    bu.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", bu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(bu.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
