#!/usr/bin/env python3
"""Generate tests/golden/partition_cases.npz by EXECUTING the reference's own function.

Runs only where the reference checkout is present (/root/reference); the output is committed.

    phasm.bubbles.partition_graph(g)                      phasm/bubbles.py:32-84, called from bubbles.py:402

run unmodified, per weakly connected component (`phasm chain` works inside one component, phasm/cli/assembler.py:289-310),
on the stand-in graph of make_components_golden plus ``is_directed`` / ``is_multigraph``, a copying ``subgraph`` as in
networkx 1.x, and ``in_edges_iter`` / ``out_edges_iter`` / ``out_edges`` that take a bunch of nodes.  Recorded per
application: the SCCs of networkx.strongly_connected_components, and per partition the node set, the edge set, the acyclic
flag and what find_superbubbles counts as sources and sinks (bubbles.py:403-406), in the canonical form of
tests/partition_utils.py (networkx yields the non-singleton SCCs in a DFS order, which is not part of the contract).

  text cases   every text case of merge_cases.npz at (b) after the cleaning chain of assembler.py:145-182 and (c) after
               merge_unambiguous_paths
  direct cases tests/partition_utils.py direct_inputs(): edges plus an explicit node order

The restatements of tests/partition_utils.py (Tarjan plus the rules, and the device's scheme run synchronously) must agree
with the reference on every application here (asserted below).

    --time    also print what networkx.strongly_connected_components takes on the paths and rings of 1 025 nodes and on the
              cleaned (b) and merged (c) graph of cfg2_1k, on this host core (best of 5 runs)"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import networkx  # noqa: E402
import numpy as np  # noqa: E402

import make_components_golden as mcg  # noqa: E402  (sets the paths up and installs the stand-in graph; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.bubbles as rb  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import components_utils as cu  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import partition_utils as pu  # noqa: E402

TIME = "--time" in sys.argv


class PartitionGraph(mcg.ChainGraph):
    def is_directed(self):
        return True

    def is_multigraph(self):
        return False

    def _bunch(self, nbunch):
        try:
            if nbunch in self.adj:
                return [nbunch]
        except TypeError:
            pass
        return [n for n in nbunch if n in self.adj]

    def subgraph(self, nbunch):
        h = PartitionGraph(**self.graph)
        for n in nbunch:
            if n in self.adj:
                h.add_node(n)
        for u in h.adj:
            for v, d in self.adj[u].items():
                if v in h.adj:
                    h.add_edge(u, v, d)
        return h

    def in_edges_iter(self, nbunch, data=False):
        for n in self._bunch(nbunch):
            for u, d in list(self.pred[n].items()):
                yield (u, n, d) if data else (u, n)

    def out_edges_iter(self, nbunch, data=False):
        for n in self._bunch(nbunch):
            for v, d in list(self.adj[n].items()):
                yield (n, v, d) if data else (n, v)

    def out_edges(self, nbunch, data=False):
        return list(self.out_edges_iter(nbunch, data))


ag.AssemblyGraph = PartitionGraph
rgfa.AssemblyGraph = PartitionGraph


def canonical(g, idx, order, weak):
    """partition_graph on every weakly connected component of g -> the canonical partitions of partition_utils."""
    rank = {n: r for r, n in enumerate(order)}
    name = lambda n: pu.R_NODE if n == "r_" else pu.RE_NODE if n == "re_" else idx(n)   # noqa: E731
    nodes_of = [[] for _ in range(weak["stats"]["n_components"])]
    for n, c in zip(g, weak["node_component"].tolist()):
        nodes_of[c].append(n)
    out = []
    for c, nodes in enumerate(nodes_of):
        component = g.subgraph(nodes)
        yielded = []
        for sub, acyclic in rb.partition_graph(component):
            num_sources = len([n for n in sub.nodes_iter() if sub.in_degree(n) == 0])      # (bubbles.py:403-406)
            num_sinks = len([n for n in sub.nodes_iter() if sub.out_degree(n) == 0])
            members = sorted((name(n) for n in sub if n not in ("r_", "re_")), key=rank.get)
            listed = members + [x for x, s in ((pu.R_NODE, "r_"), (pu.RE_NODE, "re_")) if s in sub]
            assert len(listed) == sub.number_of_nodes()
            edges = sorted((name(u), name(v)) for u, v in sub.edges_iter())
            assert len(edges) == sub.number_of_edges()
            yielded.append({"component": c, "acyclic": bool(acyclic), "nodes": listed, "edges": edges, "num_sources": num_sources,
                            "num_sinks": num_sinks})
        assert [p["acyclic"] for p in yielded] == [False] * (len(yielded) - 1) + [True], "one acyclic partition, and it comes last"
        out += sorted(yielded[:-1], key=lambda p: rank[p["nodes"][0]]) + yielded[-1:]
    return out


def nx_sccs(g, idx, order):
    """networkx.strongly_connected_components on the stand-in graph -> sorted lists of ranks, and the seconds it took."""
    rank = {n: r for r, n in enumerate(order)}
    t0 = time.perf_counter()
    comps = list(networkx.strongly_connected_components(g))
    seconds = time.perf_counter() - t0
    return sorted(sorted(rank[idx(n)] for n in c) for c in comps), seconds


def application(g, idx, totals, extra):
    """One record: the reference on g, both restatements held to it."""
    order = [idx(n) for n in g]
    edges = mdg.edge_array(g, idx)
    want_sccs, _ = nx_sccs(g, idx, order)
    weak = cu.weak_components(edges, order)
    want_parts = canonical(g, idx, order, weak)
    plain, sync = pu.partition(edges, order), pu.partition_rounds(edges, order)
    for res in (plain, sync):
        mine = {}
        for r, c in enumerate(res["node_scc"].tolist()):
            mine.setdefault(c, []).append(r)
        assert [mine[c] for c in sorted(mine)] == want_sccs, "restatement differs: SCCs"
        assert pu.reference_partitions(res, weak, edges, order) == want_parts, "restatement differs: partitions"
    for k in pu.ARRAY_KEYS:
        assert np.array_equal(plain[k], sync[k]), "the device's scheme differs: " + k
    rec = pu.record_of(plain, want_parts, edges)
    e = cu.uv_of(edges)
    rec["in_sha256"] = cu.digest(order, e[pu.by_uv(edges)])
    rec.update(extra)
    rec.update({k: sync["stats"][k] for k in ("n_trimmed", "n_outer", "n_trim_rounds", "n_forward_rounds", "n_backward_rounds")})
    totals["applications"] += 1
    for k in range(5):
        totals["class_%d" % k] += plain["stats"]["n_class"][k]
    for bit, name in ((pu.R_IN, "r_in"), (pu.RE_OUT, "re_out"), (pu.START, "start"), (pu.SINK, "sink")):
        totals["flag_" + name] += int(((plain["node_flags"] & bit) != 0).sum())
    totals["two_outer_iterations"] += sync["stats"]["n_outer"] >= 2
    totals["trim_after_a_peel"] += sync["stats"]["trim_after_peel"] > 0
    totals["empty_acyclic_partitions"] += sum(1 for p in want_parts if p["acyclic"] and not p["nodes"])
    totals["sourceless_acyclic_partitions"] += sum(1 for p in want_parts if p["acyclic"] and p["nodes"] and not p["num_sources"])
    totals["cyclic_partitions"] += sum(1 for p in want_parts if not p["acyclic"])
    totals["merged_ids"] += any(n >= extra["n_ids"] for n in order)
    totals["digest_records"] += "sha256" in rec
    return rec


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
    out["results"].append(application(g, idx0, totals, {"stage": "b", "n_ids": n_ids}))
    timed = TIME and name.endswith("cfg2_1k")
    sec_b = min(nx_sccs(g, idx0, [idx0(n) for n in g])[1] for _ in range(5)) if timed else 0.0
    ag.merge_unambiguous_paths(g)
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}
    idx = lambda n: n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)   # noqa: E731
    out["results"].append(application(g, idx, totals, {"stage": "c", "n_ids": n_ids}))
    b, cc = out["results"]
    line = "%-30s b: %5d nodes %5d SCCs (%d non-singleton, %d iterations)  c: %5d / %5d (%d, %d)" % (
        name, b["n_nodes"], b["n_sccs"], b["n_nonsingleton_sccs"], b["n_outer"], cc["n_nodes"], cc["n_sccs"], cc["n_nonsingleton_sccs"],
        cc["n_outer"])
    if timed:
        line += "  networkx: (b) %.3f ms, (c) %.3f ms (best of 5)" % (
            1e3 * sec_b, 1e3 * min(nx_sccs(g, idx, [idx(n) for n in g])[1] for _ in range(5)))
    print(line)
    return out


def direct_graph(order, edges):
    g = PartitionGraph()
    for n in order:
        g.add_node(n)
    for u, v in edges:
        g.add_edge(u, v, weight=100, overlap_len=17)
    return g


def main():
    totals = dict(applications=0, two_outer_iterations=0, trim_after_a_peel=0, empty_acyclic_partitions=0, sourceless_acyclic_partitions=0,
                  cyclic_partitions=0, merged_ids=0, digest_records=0, **{"class_%d" % k: 0 for k in range(5)},
                  **{"flag_" + k: 0 for k in ("r_in", "re_out", "start", "sink")})
    cases = []
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
    for name, order, edges, n_ids in pu.direct_inputs():
        g = direct_graph(order, edges)
        assert [n for n in g] == list(order) and sorted(g.edges_iter()) == sorted(edges)
        rec = application(g, int, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(list(order) + [-2]) + 2})
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        line = "%-40s nodes %5d  %5d SCCs  %d iterations, rounds %d / %d / %d" % (
            "direct_" + name, rec["n_nodes"], rec["n_sccs"], rec["n_outer"], rec["n_trim_rounds"], rec["n_forward_rounds"],
            rec["n_backward_rounds"])
        if TIME and (name.startswith("path_1025") or name.startswith("ring_1025")):
            line += "  networkx: %.3f ms (best of 5)" % (1e3 * min(nx_sccs(g, int, list(order))[1] for _ in range(5)))
        print(line)
    for k, v in totals.items():
        assert v > 0 or k == "digest_records", "situation %s never occurs" % k
    pu.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", pu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(pu.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
