#!/usr/bin/env python3
"""Generate tests/golden/superbubble_cases.npz by EXECUTING the reference's own functions.

Runs only where the reference checkout is present (make_merge_golden sets its path up); the output is committed.

    phasm.bubbles.partition_graph(component)                      phasm/bubbles.py:32-84
    phasm.bubbles.SuperBubbleFinderDAG(partition, report_nested)  phasm/bubbles.py:174-381, called from bubbles.py:411-414
    phasm.bubbles.superbubble_nodes(component, s, t)              phasm/bubbles.py:448-463

run unmodified, per weakly connected component, on the stand-in graph of make_partition_golden plus ``neighbors_iter`` and
``predecessors_iter``.  The finder's ``toplogical_sort`` recurses once per node of a path, so the recursion limit is raised.
The direct cases reach the finder under truthy node names (id + 1): it tests ``not start or not exit`` on the node objects
(bubbles.py:308), and the reference's own nodes are reads with a positive ``len``.

Recorded per application: the result of the contract as tests/superbubble_utils.py states it, and
from the reference, for every component whose acyclic partition has no self-loop and has both 'r_' and 're_': the pairs as a
sorted set with ``report_nested`` True, the subset reported with False, and the node set of every pair.

  text cases   every text case of merge_cases.npz at (b) after the cleaning chain of assembler.py:145-182 and (c) after
               merge_unambiguous_paths, as partition_cases.npz uses them
  direct cases tests/superbubble_utils.py direct_inputs(): those of partition_utils, then the shapes this stage is about

Asserted below: the definition by brute force equals the device's scheme run synchronously on every application small
enough; the scheme equals the reference on EVERY component that qualifies (all bubbles against report_nested=True, those
without NESTED against report_nested=False, the node_inside chains against superbubble_nodes); at least 100 applications
are compared with the reference and at least 40 of them contain a bubble.  Every direct case also goes through the finder
under two more insertion orders: where it reports the same pairs nothing is noted; where it does not (its result depends
on its DFS order on some graphs), the pairs it adds must be no superbubbles by the brute-force definition, and the case is
counted and carries them in its record.  An application with a self-loop on a singleton is pinned by the definition only.

    --time    also print what the reference's finder takes (partition_graph not included) on the paths of 1 025 nodes and
              on the cleaned (b) and merged (c) graph of cfg2_1k, on this host core (best of 5 runs)"""
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.setrecursionlimit(20000)

import numpy as np  # noqa: E402

import make_partition_golden as mpg  # noqa: E402  (sets the paths up and installs the stand-in graph; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.bubbles as rb  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import components_utils as cu  # noqa: E402
import diamond_utils as du  # noqa: E402
import make_diamond_golden as mdg  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import superbubble_utils as su  # noqa: E402

TIME = "--time" in sys.argv


class SuperbubbleGraph(mpg.PartitionGraph):
    def subgraph(self, nbunch):
        h = SuperbubbleGraph(**self.graph)
        for n in nbunch:
            if n in self.adj:
                h.add_node(n)
        for u in h.adj:
            for v, d in self.adj[u].items():
                if v in h.adj:
                    h.add_edge(u, v, d)
        return h

    def neighbors_iter(self, n):
        return iter(list(self.adj[n]))

    def predecessors_iter(self, n):
        return iter(list(self.pred[n]))


ag.AssemblyGraph = SuperbubbleGraph
rgfa.AssemblyGraph = SuperbubbleGraph


def reference(g, idx, order, weak, seconds=None):
    """The reference on every component of g that qualifies -> (component numbers, sorted pairs with nesting reported, sorted
    pairs without, the sorted node set of every pair of the first list), node ids by ``idx``; the other components by reason."""
    nodes_of = [[] for _ in range(weak["stats"]["n_components"])]
    for n, c in zip(g, weak["node_component"].tolist()):
        nodes_of[c].append(n)
    compared, pairs, top, sets, skipped = [], [], [], [], {"self_loop": 0, "no_singletons": 0}
    for c, nodes in enumerate(nodes_of):
        component = g.subgraph(nodes)
        partition, acyclic = list(rb.partition_graph(component))[-1]
        assert acyclic
        real = [n for n in partition if n not in ("r_", "re_")]
        if any(partition.has_edge(n, n) for n in real):
            skipped["self_loop"] += 1
            continue
        if "r_" not in partition or "re_" not in partition:
            assert not real, "a loop-free acyclic partition with a node has a source and a sink"
            skipped["no_singletons"] += 1
            continue
        t0 = time.perf_counter()
        found = list(rb.SuperBubbleFinderDAG(partition, True))
        found_top = list(rb.SuperBubbleFinderDAG(partition, False))
        if seconds is not None:
            seconds.append(time.perf_counter() - t0)
        assert len(set(found)) == len(found) and set(found_top) <= set(found)
        compared.append(c)
        for s, t in found:
            pairs.append((idx(s), idx(t)))
            sets.append(sorted(idx(n) for n in rb.superbubble_nodes(component, s, t)))
        top += [(idx(s), idx(t)) for s, t in found_top]
    by = sorted(range(len(pairs)), key=lambda i: pairs[i])
    return compared, [pairs[i] for i in by], sorted(top), [sets[i] for i in by], skipped


def application(g, idx, totals, extra, seconds=None):
    """One record: the contract by the scheme (and, where small enough, by brute force), held to the reference."""
    order = [idx(n) for n in g]
    edges = mdg.edge_array(g, idx)
    weak = cu.weak_components(edges, order)
    sync = su.scheme(edges, order)
    brute = len(order) <= su.BRUTE_FORCE_UP_TO
    if brute:
        plain = su.definition(edges, order)
        for k in su.ARRAY_KEYS:
            assert np.array_equal(plain[k], sync[k]), "the scheme differs from the definition: " + k
        assert {k: plain["stats"][k] for k in su.STAT_KEYS} == {k: sync["stats"][k] for k in su.STAT_KEYS}
    compared, ref_pairs, ref_top, ref_sets, skipped = reference(g, idx, order, weak, seconds)
    comp_of = dict(zip(order, weak["node_component"].tolist()))
    mine = [(s, t, nested, nodes) for s, t, nested, nodes in zip(sync["b_entrance"].tolist(), sync["b_exit"].tolist(),
                                                                  sync["b_nested"].tolist(), su.node_sets(sync, order))
            if comp_of[s] in set(compared)]
    assert sorted((s, t) for s, t, _, _ in mine) == ref_pairs, "the scheme differs from the reference: pairs"
    assert sorted((s, t) for s, t, nested, _ in mine if not nested) == ref_top, "the scheme differs from the reference: not nested"
    assert [nodes for _, _, _, nodes in sorted(mine)] == ref_sets, "the scheme differs from the reference: superbubble_nodes"
    if skipped["self_loop"] == 0:
        assert len(mine) == sync["stats"]["n_bubbles"], "a component without singletons has no bubble"
    rec = su.record_of(sync)
    e = cu.uv_of(edges)
    rec["in_sha256"] = cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))])
    rec.update(extra)
    rec.update({k: sync["stats"][k] for k in su.SCHEME_KEYS})
    rec["ref_components"] = compared
    rec["ref_skipped_self_loop"] = skipped["self_loop"]
    if rec["n_edges"] > su.DIGEST_ABOVE:
        rec["ref_sha256"] = cu.digest(ref_pairs, ref_top, [len(x) for x in ref_sets], [n for x in ref_sets for n in x])
    else:
        rec["ref_pairs"] = [x for p in ref_pairs for x in p]
        rec["ref_top"] = [x for p in ref_top for x in p]
        rec["ref_set_sizes"] = [len(x) for x in ref_sets]
        rec["ref_set_nodes"] = [n for x in ref_sets for n in x]
    st = sync["stats"]
    whole = bool(compared) and skipped["self_loop"] == 0
    totals["applications"] += 1
    totals["compared_with_the_reference"] += whole
    totals["compared_and_with_a_bubble"] += whole and bool(ref_pairs)
    totals["reference_pairs"] += len(ref_pairs)
    totals["pinned_by_the_definition_only"] += skipped["self_loop"] > 0
    totals["brute_forced"] += brute
    totals["nested"] += st["n_nested"]
    totals["discarded"] += st["n_discarded"]
    totals["self_loop_nodes"] += st["n_self_loop_nodes"]
    totals["exit_is_an_entrance"] += int(((sync["node_flags"] & 3) == 3).sum())
    totals["not_nested_inside_a_discarded_one"] += st["n_survivors_in_discarded"]
    totals["several_discard_rounds"] += st["n_discard_rounds"] > 1
    totals["several_components"] += weak["stats"]["n_components"] > 1
    totals["components_without_singletons"] += skipped["no_singletons"]
    totals["max_levels"] = max(totals["max_levels"], st["n_levels_forward"])
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
    timed = TIME and name.endswith("cfg2_1k")
    out["results"].append(application(g, idx0, totals, {"stage": "b", "n_ids": n_ids}))
    sec_b = best_of_5(g, idx0) if timed else 0.0
    ag.merge_unambiguous_paths(g)
    merged = [n for n in g if isinstance(n, MergedReads)]
    k_of = {str(n): k for k, n in enumerate(merged)}
    idx = lambda n: n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)   # noqa: E731
    out["results"].append(application(g, idx, totals, {"stage": "c", "n_ids": n_ids}))
    b, cc = out["results"]
    line = "%-30s b: %5d nodes %4d bubbles (%d nested, %d levels)  c: %5d / %4d (%d, %d)" % (
        name, b["n_nodes"], b["n_bubbles"], b["n_nested"], b["n_levels_forward"], cc["n_nodes"], cc["n_bubbles"], cc["n_nested"],
        cc["n_levels_forward"])
    if timed:
        line += "  the reference's finder: (b) %.3f ms, (c) %.3f ms (best of 5)" % (1e3 * sec_b, 1e3 * best_of_5(g, idx))
    print(line)
    return out


def best_of_5(g, idx):
    order = [idx(n) for n in g]
    weak = cu.weak_components(mdg.edge_array(g, idx), order)
    runs = []
    for _ in range(5):
        seconds = []
        reference(g, idx, order, weak, seconds)
        runs.append(sum(seconds))
    return min(runs)


def direct_graph(order, edges):
    """The direct case under truthy node names: node id + 1."""
    g = SuperbubbleGraph()
    for n in order:
        g.add_node(n + 1)
    for u, v in edges:
        g.add_edge(u + 1, v + 1, weight=100, overlap_len=17)
    return g


def main():
    keys = ("applications", "compared_with_the_reference", "compared_and_with_a_bubble", "reference_pairs", "pinned_by_the_definition_only",
            "brute_forced", "nested", "discarded", "self_loop_nodes", "exit_is_an_entrance", "not_nested_inside_a_discarded_one",
            "several_discard_rounds", "several_components", "components_without_singletons", "max_levels", "digest_records",
            "direct_cases_where_the_finder_depends_on_the_order")
    totals = {k: 0 for k in keys}
    idx = lambda n: n - 1   # noqa: E731
    cases = []
    for c in mu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
    for name, order, edges, n_ids in su.direct_inputs():
        g = direct_graph(order, edges)
        assert [idx(n) for n in g] == list(order) and sorted((idx(u), idx(v)) for u, v in g.edges_iter()) == sorted(edges)
        rec = application(g, idx, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(list(order) + [-2]) + 2})
        # the finder is deterministic: the same pairs whatever the insertion order of nodes and edges
        seen = []
        for k in range(3):
            o, e = (list(order), list(edges)) if k == 0 else (list(order)[::-1], list(edges)[::-1]) if k == 1 else \
                (sorted(order, key=lambda x: random.Random(x).random()), sorted(edges, key=lambda x: random.Random(hash(x)).random()))
            h = direct_graph(o, e)
            w = cu.weak_components(mdg.edge_array(h, idx), [idx(n) for n in h])
            _, pairs, top, sets, _ = reference(h, idx, [idx(n) for n in h], w)
            seen.append((pairs, top, sets))
        if not seen[0] == seen[1] == seen[2]:
            # The finder is NOT deterministic on this case: under another insertion order its DFS numbers the nodes
            # differently and it reports other pairs.  The order of the case itself is held to the definition above (brute
            # force, the scheme and the reference agree there); what another order adds or drops is checked against the
            # definition here, counted, and named in the record.
            assert len(order) <= su.BRUTE_FORCE_UP_TO, "only a brute-forced case can settle what the finder disagrees with itself about"
            truth = set(seen[0][0])
            odd = sorted(set().union(*[set(s[0]) ^ truth for s in seen[1:]]))
            assert odd and all(p not in truth for p in odd), "under another order the finder drops a superbubble: " + name
            rec["ref_order_dependent_pairs"] = [x for p in odd for x in p]
            totals["direct_cases_where_the_finder_depends_on_the_order"] += 1
            print("    the finder reports %s only under another insertion order: not superbubbles by the definition" % odd)
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        line = "%-50s nodes %5d  %4d bubbles (%d nested, %d discarded)  levels %d / %d" % (
            "direct_" + name, rec["n_nodes"], rec["n_bubbles"], rec["n_nested"], rec["n_discarded"], rec["n_levels_forward"],
            rec["n_levels_backward"])
        if TIME and name.startswith("sb_path_1025"):
            line += "  the reference's finder: %.3f ms (best of 5)" % (1e3 * best_of_5(g, idx))
        print(line)
    for k, v in totals.items():
        assert v > 0 or k in ("digest_records", "direct_cases_where_the_finder_depends_on_the_order"), "situation %s never occurs" % k
    assert totals["compared_with_the_reference"] >= 100 and totals["compared_and_with_a_bubble"] >= 40, totals
    assert totals["max_levels"] >= 1025
    su.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", su.GOLDEN_FILE, len(cases), "cases", os.path.getsize(su.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
