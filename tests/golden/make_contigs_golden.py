#!/usr/bin/env python3
"""Generate tests/golden/contig_cases.npz by EXECUTING the reference's own function.

Runs only where the reference checkout is present (make_merge_golden sets its path up); the output is committed.

    phasm.assembly_graph.identify_contigs(g, exclude_nodes, min_contig_len)      phasm/assembly_graph.py:655-718

run unmodified on the stand-in graph of make_bubblechains_golden, which keeps the order of its nodes and edges.  The stand-in
has no ``path_length`` of the reference's class; it is taken, unmodified, from a second copy of the reference's module that is
loaded under another name before this process imports anything that points the module's ``AssemblyGraph`` at a stand-in.
The reference's ``node_path_edges`` cannot be taken the same way: it is a generator that ends by letting ``next()`` raise
StopIteration inside its body, which since PEP 479 (Python 3.7) is a RuntimeError.  The stand-in keeps the restatement
make_tips_golden.TipsGraph has had for that reason since the tip stage (the same tuples, ended by ``return``).  The function
is local (a path never leaves its weakly connected component), so it runs on the
whole graph at once; `phasm chain` runs it per component and gets the union.

Recorded per application: the result of the contract as tests/contig_utils.py states it, and from the
reference the paths it yields, as a sorted list of node tuples.

  text cases   every text case of merge_cases.npz at (b) after the cleaning chain of assembler.py:145-182 and (c) after
               merge_unambiguous_paths, with X = the nodes that carry a chain in bubblechain_utils.scheme (min_nodes 1), for
               min_contig_len 5000 and 0
  direct cases tests/contig_utils.py direct_inputs()

Asserted below: the restated walk (``definition``) equals the device's scheme run synchronously (``scheme``) in every array
on every application; the reference's paths equal the definition's as sorted lists of node tuples on EVERY application; no
path is reported twice; every situation of ``SITUATIONS`` occurs.

    --time    also print what the reference's identify_contigs takes on the paths of 1 025 nodes and on the cleaned (b) and
              merged (c) graph of cfg2_1k, on this host core (best of 5 runs)"""
import importlib.util
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

# the reference's class as its module defines it: a second copy under another name, loaded first
_spec = importlib.util.spec_from_file_location("phasm_assembly_graph_pristine", "/root/reference/phasm/assembly_graph.py")
pristine = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pristine)

import numpy as np  # noqa: E402

import make_bubblechains_golden as mbg  # noqa: E402  (sets the paths up, installs the stand-in graph, raises the recursion limit)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import bubblechain_utils as bu  # noqa: E402
import components_utils as cu  # noqa: E402
import contig_utils as ct  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import superbubble_utils as su  # noqa: E402

TIME = "--time" in sys.argv
SITUATIONS = ("covered_late_start", "uncovered_ring", "blocked_start", "path_through_excluded_nodes", "path_ending_at_its_first_node",
              "reported_isolated_node", "dropped_isolated_node", "sum_above_32_bits")


class ContigGraph(mbg.BubblechainGraph):
    path_length = pristine.AssemblyGraph.path_length                # the reference's own (node_path_edges: see above)


assert ContigGraph.path_length.__code__.co_filename.startswith("/root/reference/")


class LNode(mdg.M):
    """A node of a direct case with a length of its own."""
    lengths = {}

    def __len__(self):
        return LNode.lengths[int(self)]

    def __bool__(self):
        return True


def reference(g, idx, exclude, min_len):
    """The reference on g -> the paths it yields, as a sorted list of node-id tuples."""
    X = {n for n in g if idx(n) in exclude}
    return sorted(tuple(idx(n) for n in path) for path in ag.identify_contigs(g, X, min_len))


def application(g, idx, totals, extra, exclude, min_len):
    order = [idx(n) for n in g]
    edges = mdg.edge_array(g, idx)
    lengths = {idx(n): len(n) for n in g}
    plain = ct.definition(edges, order, lengths, exclude, min_len)
    sync = ct.scheme(edges, order, lengths, exclude, min_len)
    for k in ct.ARRAY_KEYS:
        assert np.array_equal(plain[k], sync[k]), "the scheme differs from the definition: " + k
    assert {k: plain["stats"][k] for k in ct.STAT_KEYS} == {k: sync["stats"][k] for k in ct.STAT_KEYS}
    path_bound, cover_bound = ct.round_bounds(sync["stats"])
    assert sync["stats"]["n_path_rounds"] <= path_bound and sync["stats"]["n_cover_rounds"] <= cover_bound
    ref_paths = reference(g, idx, set(exclude), min_len)
    mine = sorted(ct.paths_of(plain, edges))
    assert mine == ref_paths, "the definition differs from the reference"
    assert len(set(ref_paths)) == len(ref_paths), "a path is reported twice"
    rec = ct.record_of(sync, edges)
    e = cu.uv_of(edges)
    by = np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, np.int64)
    rec["in_sha256"] = cu.digest(order, e[by], np.asarray(edges, np.int64).reshape(-1, 4)[by, 2], [lengths[n] for n in order], sorted(exclude))
    rec.update(extra)
    rec["min_contig_len"] = min_len
    rec.update({k: sync["stats"][k] for k in ct.SCHEME_KEYS})
    flat = [n for p in ref_paths for n in p]
    if rec["n_edges"] > ct.DIGEST_ABOVE:
        rec["ref_sha256"] = cu.digest([len(p) for p in ref_paths], flat)
    else:
        rec["ref_path_sizes"] = [len(p) for p in ref_paths]
        rec["ref_path_nodes"] = flat
    st = sync["stats"]
    X = set(exclude)
    totals["applications"] += 1
    totals["reference_paths"] += len(ref_paths)
    indeg = {}
    for v in e[:, 1].tolist():
        indeg[v] = indeg.get(v, 0) + 1
    totals["covered_late_start"] += any(len(p) > 1 and indeg.get(p[0], 0) == 1 for p in ref_paths)   # (a root start leaves in != 1)
    totals["uncovered_ring"] += st["n_uncovered_edges"] > 0 and st["n_blocked"] == 0
    totals["blocked_start"] += st["n_blocked"] > 0
    totals["path_through_excluded_nodes"] += any(len(p) > 2 and any(n in X for n in p[1:-1]) and p[0] not in X for p in ref_paths)
    totals["path_ending_at_its_first_node"] += any(len(p) > 1 and p[0] == p[-1] for p in ref_paths)
    totals["reported_isolated_node"] += st["n_isolated"] > st["n_short_isolated"]
    totals["dropped_isolated_node"] += st["n_short_isolated"] > 0
    totals["sum_above_32_bits"] += any(x >= 2**32 for x in sync["c_length"].tolist())
    totals["max_path_rounds"] = max(totals["max_path_rounds"], st["n_path_rounds"])
    totals["max_cover_rounds"] = max(totals["max_cover_rounds"], st["n_cover_rounds"])
    totals["digest_records"] += "sha256" in rec
    return rec


def best_of_5(g, idx, exclude, min_len):
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        reference(g, idx, exclude, min_len)
        runs.append(time.perf_counter() - t0)
    return min(runs)


def chain_nodes(g, idx):
    """X as `phasm chain` builds it, by the restatement of the bubble-chain stage: the nodes that carry a chain."""
    order = [idx(n) for n in g]
    edges = mdg.edge_array(g, idx)
    res = bu.scheme(edges, order, 1, su.scheme(edges, order))
    return sorted(int(n) for n, c in zip(order, res["node_chain"].tolist()) if c != bu.NONE)


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
    X = chain_nodes(g, idx0)
    for min_len in (5000, 0):
        out["results"].append(application(g, idx0, totals, {"stage": "b", "n_ids": n_ids, "exclude": X}, X, min_len))
    sec_b = best_of_5(g, idx0, set(X), 5000) if timed else 0.0
    ag.merge_unambiguous_paths(g)
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}
    idx = lambda n: n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)   # noqa: E731
    X = chain_nodes(g, idx)
    for min_len in (5000, 0):
        out["results"].append(application(g, idx, totals, {"stage": "c", "n_ids": n_ids, "exclude": X}, X, min_len))
    b, cc = out["results"][1], out["results"][3]
    line = "%-30s b: %5d nodes %4d excluded %4d contigs  c: %5d / %4d / %4d" % (
        name, b["n_nodes"], b["n_excluded"], b["n_contigs"], cc["n_nodes"], cc["n_excluded"], cc["n_contigs"])
    if timed:
        line += "  the reference's identify_contigs: (b) %.3f ms, (c) %.3f ms (best of 5)" % (1e3 * sec_b, 1e3 * best_of_5(g, idx, set(X), 5000))
    print(line)
    return out


def direct_graph(order, edges, lengths):
    """The direct case under truthy node names: node id + 1."""
    LNode.lengths = {n + 1: x for n, x in lengths.items()}
    g = ContigGraph()
    for n in order:
        g.add_node(LNode(n + 1))
    for u, v, w in edges:
        g.add_edge(LNode(u + 1), LNode(v + 1), weight=w, overlap_len=17)
    return g


def main():
    ag.AssemblyGraph = ContigGraph
    mbg.msg.rgfa.AssemblyGraph = ContigGraph
    keys = ("applications", "reference_paths") + SITUATIONS + ("max_path_rounds", "max_cover_rounds", "digest_records")
    totals = {k: 0 for k in keys}
    idx = lambda n: int(n) - 1   # noqa: E731
    cases = []
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
    print("the text cases alone:", totals)
    for name, order, edges, lengths, exclude, min_len in ct.direct_inputs():
        g = direct_graph(order, edges, lengths)
        assert [idx(n) for n in g] == list(order) and sorted((idx(u), idx(v)) for u, v in g.edges_iter()) == sorted((u, v) for u, v, _ in edges)
        rec = application(g, idx, totals, {"stage": "a", "n_ids": max(list(order) + [-2]) + 2}, exclude, min_len)
        cases.append({"name": "direct_" + name, "direct": True, "results": [rec]})
        line = "%-50s nodes %5d  %4d starts, %4d paths, %4d contigs, %4d uncovered, rounds %d + %d" % (
            "direct_" + name, rec["n_nodes"], rec["n_root_starts"] + rec["n_late_starts"], rec["n_paths"], rec["n_contigs"],
            rec["n_uncovered_edges"], rec["n_path_rounds"], rec["n_cover_rounds"])
        if TIME and name.startswith("path_1025"):
            line += "  the reference's identify_contigs: %.3f ms (best of 5)" % (1e3 * best_of_5(g, idx, set(exclude), min_len))
        print(line)
    for k, v in totals.items():
        assert v > 0 or k == "digest_records", "situation %s never occurs" % k
    assert totals["max_path_rounds"] > 8 and totals["max_cover_rounds"] > 8, totals       # both loops cross a batch
    ct.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", ct.GOLDEN_FILE, len(cases), "cases", os.path.getsize(ct.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
