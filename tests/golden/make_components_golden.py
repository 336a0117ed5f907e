#!/usr/bin/env python3
"""Generate tests/golden/components_cases.npz.

Runs only where the reference checkout is present (/root/reference); the output is committed.

The first step of `phasm chain` (phasm/cli/assembler.py:231-310) is networkx's weakly_connected_component_subgraphs on the
graph that gfa2_parse_segments_with_fragments and gfa2_reconstruct_assembly_graph (phasm/io/gfa.py:112-227) rebuild from
the file `phasm layout` wrote.  The reference was written for networkx 1.x; the 3.4 installed here yields the components
by the same rule (``for v in G: if v not in seen: yield bfs(v)``), and only 3.4 can be executed here.

  text cases   every text case of merge_cases.npz (the union, ring and lasso cases with it): the components, computed by
               networkx.weakly_connected_components on a DiGraph with the reference graph's node insertion order and edges,
               (a) of the stage-1 graph, (b) after the cleaning chain of assembler.py:145-182, (c) after merge_unambiguous_paths
  file route   at (c) the file the reference's gfa2_write_graph writes, read back by the reference's two functions,
               unmodified, on the stand-in graph of make_merge_golden: node order, edges, components, and a digest of what
               the reference's gfa2_write_graph and gfa1_write_graph write for g.subgraph(component) of every component
  hand files   the graph files of tests/components_utils.py HAND_FILES, through the same two functions
  direct cases tests/components_utils.py direct_inputs(): edges plus an explicit node order

The restatements of tests/components_utils.py, the reader of phasm_amd/io/gfa.py and the writers of phasm_amd/layout.py
must agree with the reference on every application here (asserted below).

    --time    also print what networkx takes on the stage-(b) and stage-(c) graphs of cfg2_1k, on this host core"""
import io
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import networkx  # noqa: E402
import numpy as np  # noqa: E402

import make_merge_golden as mmg  # noqa: E402  (sets the paths up and installs the stand-in graph; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import components_utils as cu  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import tips_utils as tu  # noqa: E402
from phasm_amd import layout as my_layout  # noqa: E402
from phasm_amd.io import gfa as my_gfa  # noqa: E402

TIME = "--time" in sys.argv


class ChainGraph(mmg.MergeGraph):
    """... plus ``subgraph`` as networkx 1.x builds it: the nodes in the order of the bunch, every edge between them."""

    def subgraph(self, nbunch):
        h = ChainGraph(**self.graph)
        for n in nbunch:
            if n in self.adj:
                h.add_node(n)
        for u in h.adj:
            for v, d in self.adj[u].items():
                if v in h.adj:
                    h.add_edge(u, v, d)
        return h


ag.AssemblyGraph = ChainGraph
rgfa.AssemblyGraph = ChainGraph   # (phasm.io.gfa binds the name at import)


def nx_components(order, uv):
    """networkx.weakly_connected_components on a DiGraph with this node insertion order -> a weak_components-shaped result."""
    G = networkx.DiGraph()
    G.add_nodes_from(order)
    G.add_edges_from(uv)
    t0 = time.perf_counter()
    comps = list(networkx.weakly_connected_components(G))
    seconds = time.perf_counter() - t0
    of = {}
    for i, c in enumerate(comps):
        for n in c:
            of[n] = i
    rank = {n: r for r, n in enumerate(order)}
    first = [min(c, key=rank.get) for c in comps]
    assert [rank[f] for f in first] == sorted(rank[f] for f in first), "networkx numbers by the lowest-ranked node"
    node_comp = np.asarray([of[n] for n in order], dtype=np.int64)
    edge_comp = np.asarray([of[u] for u, _ in uv], dtype=np.int64)
    assert all(of[u] == of[v] for u, v in uv)
    K = len(comps)
    n_nodes, n_edges = np.bincount(node_comp, minlength=K).astype(np.int64), np.bincount(edge_comp, minlength=K).astype(np.int64)
    if K == 0:
        n_nodes = n_edges = np.zeros(0, np.int64)
    # what the reference logs per component: number_of_nodes / number_of_edges of the subgraph
    for i, c in enumerate(comps[:50]):
        sub = G.subgraph(c)
        assert (sub.number_of_nodes(), sub.number_of_edges()) == (int(n_nodes[i]), int(n_edges[i]))
    stats = {"n_nodes": len(order), "n_edges": len(uv), "n_components": K, "n_singletons": int((n_nodes == 1).sum()),
             "max_component_nodes": int(n_nodes.max()) if K else 0, "max_component_edges": int(n_edges.max()) if K else 0}
    return {"node_component": node_comp, "edge_component": edge_comp, "first_node": np.asarray(first, dtype=np.int64),
            "n_nodes": n_nodes, "n_edges": n_edges, "stats": stats}, seconds


KEYS = ("node_component", "edge_component", "first_node", "n_nodes", "n_edges")


def application(order, edges, totals, extra=None):
    """One record: networkx on (order, edges), both restatements held to it."""
    uv = [(int(e[0]), int(e[1])) for e in edges]
    want, seconds = nx_components(order, uv)
    mine, sync = cu.weak_components(uv, order), cu.components_rounds(uv, order)
    for res in (mine, sync):
        for k in KEYS:
            assert np.array_equal(res[k], want[k]), "restatement differs: " + k
        assert {k: res["stats"][k] for k in cu.STAT_KEYS} == want["stats"]
    rec = cu.record_of(want, sync["stats"]["rounds"])
    e = np.asarray([list(x)[:2] for x in edges], dtype=np.int64).reshape(-1, 2)
    rec["in_sha256"] = cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))])
    rec.update(extra or {})
    st = want["stats"]
    totals["applications"] += 1
    totals["singletons"] += st["n_singletons"]
    totals["self_loops"] += sum(u == v for u, v in uv)
    totals["several_components"] += st["n_components"] > 1
    totals["interleaved_ranks"] += bool(np.any(np.diff(want["node_component"]) < 0))
    totals["merged_ids"] += bool(extra and any(n >= extra.get("n_ids", 1 << 62) for n in order))
    totals["max_rounds"] = max(totals["max_rounds"], rec["rounds"])
    totals["digest_records"] += "sha256" in rec
    return rec, seconds


def reference_file_route(text, totals):
    """The reference's two functions on a graph file -> (record, None) or (None, which function raised)."""
    try:
        reads = rgfa.gfa2_parse_segments_with_fragments(io.StringIO(text))
    except Exception as exc:   # noqa: BLE001
        return None, {"raises": "gfa2_parse_segments_with_fragments", "error": type(exc).__name__}
    try:
        g = rgfa.gfa2_reconstruct_assembly_graph(io.StringIO(text), reads)
    except Exception as exc:   # noqa: BLE001
        return None, {"raises": "gfa2_reconstruct_assembly_graph", "error": type(exc).__name__}
    graph = my_gfa.read_graph_gfa(text.splitlines(True))
    idx = lambda n: 2 * graph.names.index(str(n)[:-1]) + (str(n)[-1] == "-")   # noqa: E731
    order = [idx(n) for n in g]
    edges = [[idx(u), idx(v), int(d["weight"]), int(d["overlap_len"])] for u, v, d in g.edges_iter(data=True)]
    # the reader of phasm_amd/io/gfa.py against the reference's reconstruction
    assert graph.node_order == order, "read_graph_gfa: node order differs"
    assert sorted(graph.edges.tolist()) == sorted(edges), "read_graph_gfa: edges differ"
    for n in g:
        assert graph.node_length(idx(n)) == len(n)
        if isinstance(n, MergedReads):
            assert (list(n.reads), list(n.prefix_lengths)) == tuple(map(list, graph.fragments[idx(n) >> 1])) or \
                ([str(r) for r in n.reads], list(n.prefix_lengths)) == [list(x) for x in graph.fragments[idx(n) >> 1]]
    want, _ = nx_components(order, [(e[0], e[1]) for e in edges])
    mine = cu.weak_components(graph.edges, graph.node_order)
    for k in ("node_component", "first_node", "n_nodes", "n_edges"):
        assert np.array_equal(mine[k], want[k]), "file route, restatement differs: " + k
    rec = cu.graph_file_record(graph, want)
    nodes_of = {i: [] for i in range(want["stats"]["n_components"])}
    for n, c in zip(g, want["node_component"].tolist()):
        nodes_of[c].append(n)
    ref_written, my_written = [], []
    for i, nodes in nodes_of.items():
        sub = g.subgraph(set(nodes))
        out = []
        for writer in (rgfa.gfa2_write_graph, rgfa.gfa1_write_graph):
            f = io.StringIO()
            writer(f, sub)
            out.append(f.getvalue().splitlines(True))
        ref_written.append(out)
        e_idx = np.flatnonzero(mine["edge_component"] == i)
        my_nodes = [n for n, c in zip(graph.node_order, mine["node_component"].tolist()) if c == i]
        my_written.append((my_layout.component_gfa2_lines(graph, my_nodes, graph.edges[e_idx]),
                           my_layout.component_gfa1_lines(graph, my_nodes, graph.edges[e_idx])))
    rec["writers_sha256"] = cu.writers_digest(ref_written)
    assert cu.writers_digest(my_written) == rec["writers_sha256"], "the component writers differ from the reference's"
    totals["file_routes"] += 1
    totals["file_merged_nodes"] += sum(isinstance(n, MergedReads) for n in g)
    totals["file_segments_without_edges"] += sum(1 for n in g if not g.adj[n] and not g.pred[n])
    return rec, None


def text_case(c, totals):
    name, params = c["name"], c["params"]
    text = mu.case_text(c)
    out = {k: c[k] for k in ("reduce_case", "synth", "text_sha256") if k in c}
    out.update(name=name, params=params, results=[])
    g, node_index = mrg.stage1_graph(text, params)
    idx0 = lambda n: node_index[str(n)]   # noqa: E731
    n_ids = len(node_index)
    lengths = np.zeros(n_ids, dtype=np.int64)
    for n in g:
        lengths[idx0(n)] = len(n)
    rec, _ = application([idx0(n) for n in g], mdg.edge_array(g, idx0), totals, {"stage": "a", "n_ids": n_ids})
    out["results"].append(rec)
    g.remove_edges_from(ag.remove_transitive_edges(g, du.STAGE_FUZZ))
    ag.make_symmetric(g)
    ag.remove_tips(g, du.STAGE_L, du.STAGE_B)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    ag.remove_diamond_tips(g)
    ag.remove_tips(g, du.STAGE_L)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    order_b, e_b = [idx0(n) for n in g], mdg.edge_array(g, idx0)
    rec, sec_b = application(order_b, e_b, totals, {"stage": "b", "n_ids": n_ids})
    out["results"].append(rec)
    ag.merge_unambiguous_paths(g)
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}
    idx = lambda n: n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)   # noqa: E731
    rec, sec_c = application([idx(n) for n in g], mdg.edge_array(g, idx), totals, {"stage": "c", "n_ids": n_ids})
    out["results"].append(rec)
    # the file route: the file the reference writes for (c), as a permutation of the E lines tests/merge_utils.py restates
    f = io.StringIO()
    rgfa.gfa2_write_graph(f, g)
    lines = f.getvalue().splitlines(True)
    head, e_lines = [l for l in lines if l[0] != "E"], [l for l in lines if l[0] == "E"]
    names = {i: s for s, i in node_index.items()}
    my_head, my_e = mu.gfa_lines(mu.merge_paths(e_b[tu.by_uv(e_b)], order_b, lengths, n_ids), names, lengths, n_ids)
    assert my_head == head and sorted(my_e) == sorted(e_lines) and len(set(my_e)) == len(my_e)
    at = {l: i for i, l in enumerate(my_e)}
    frec, raised = reference_file_route("".join(lines), totals)
    out["file"] = dict(frec if frec is not None else raised, e_perm=[at[l] for l in e_lines], text_sha256=mu.lines_digest(lines))
    a, b, cc = out["results"]
    print("%-30s a: %6d nodes %5d components (%d rounds)  b: %5d / %4d (%d)  c: %5d / %4d (%d)  file: %s%s" % (
        name, a["n_nodes"], a["n_components"], a["rounds"], b["n_nodes"], b["n_components"], b["rounds"], cc["n_nodes"],
        cc["n_components"], cc["rounds"], "%d components" % frec["n_components"] if frec else raised["raises"],
        "  networkx: b %.2f ms, c %.2f ms" % (1e3 * sec_b, 1e3 * sec_c) if TIME else ""))
    return out


def main():
    totals = dict(applications=0, singletons=0, self_loops=0, several_components=0, interleaved_ranks=0, merged_ids=0, max_rounds=0,
                  digest_records=0, file_routes=0, file_merged_nodes=0, file_segments_without_edges=0, hand_raises=0)
    cases = []
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
    hand = []
    for name, text in cu.HAND_FILES.items():
        frec, raised = reference_file_route(text, totals)
        totals["hand_raises"] += raised is not None
        hand.append(dict(frec if frec is not None else raised, name=name))
        print("hand file %-40s %s" % (name, "%d nodes, %d components" % (frec["n_nodes"], frec["n_components"]) if frec else raised))
    for name, order, edges, n_ids in cu.direct_inputs():
        rec, _ = application(order, edges, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(order + [-2]) + 2})
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        print("%-50s nodes %6d  %5d components (%d rounds)" % ("direct_" + name, rec["n_nodes"], rec["n_components"], rec["rounds"]))
    for k in ("singletons", "self_loops", "several_components", "interleaved_ranks", "merged_ids", "digest_records", "file_routes",
              "file_merged_nodes", "file_segments_without_edges"):
        assert totals[k] > 0, "situation %s never occurs" % k
    assert totals["max_rounds"] >= 13
    cu.save_golden({"totals": totals, "cases": cases, "hand_files": hand})
    print("totals", totals)
    print("wrote", cu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(cu.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
