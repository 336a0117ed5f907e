#!/usr/bin/env python3
"""Generate tests/golden/superbubble_all_cases.npz: the contract of po_layout_superbubbles_all on
every application.  Needs neither a GPU nor the reference checkout; the output is committed.

The contract restated.  A pair (s, t), s != t, is a superbubble iff (1) t is reachable from s, (2) the set U reached from s
without passing t equals the set that reaches t without passing s, (3) G[U] is acyclic -- a self-loop on a member and an
edge t -> s are cycles -- and (4) no other t' in U satisfies (1)-(3) with s.  The scheme restated.  Splitting a node x gives
x_out, a source with all out-edges of x, and x_in, a sink with ALL in-edges of x.  The superbubbles of G that do not hold x
strictly inside are those of G with x split, after renaming the copies back, dropping (x_out, x_in) and dropping every
(s, t) with an edge t -> s.  A node with an in-edge from outside its SCC (R_IN) can only be an entrance, one with an
out-edge to outside (RE_OUT) only an exit, so per level every non-singleton SCC of the current flat graph splits its
lowest-ranked R_IN node, else its lowest-ranked RE_OUT node; an SCC of the split graph always has an R_IN node.  Levels
until no non-singleton SCC is left, then the stage of section 3.9j on the flat graph.  An SCC with neither (a whole weak
component: ROOTLESS) splits its lowest rank x; x is CERTIFIED iff that alone leaves no cycle in the SCC (x lies on every
cycle, so it is strictly inside no bubble).  Otherwise the nodes of one shortest cycle through x root one more run each,
up to the first certified one: a bubble is missed only by a root strictly inside it, and no cycle lies inside one bubble.
The runs are merged: pairs by union, node_inside by the smallest n_inside.

Asserted on EVERY application whose weakly connected components have at most 300 nodes:
    definition_all == by_partition == scheme_all in every array and count (the partition theorem and the scheme)
and on every application, whatever its size:
    the entries on singleton nodes equal superbubble_utils' restatement of po_layout_superbubbles, and that call reports
    nothing on the other nodes.

  direct cases  tests/cyclic_utils.py direct_inputs(): the shapes this call is about, then those of superbubble_utils
  text cases    every text case of partition_cases.npz at (b) after the cleaning chain and (c) after
                merge_unambiguous_paths, as tests/test_partition_oracle.py rebuilds them

The reference's own route (graph_to_dag plus SuperBubbleFinder) is not executed: under the installed networkx its
graph_to_dag fails at ``dfs_tree(...).nodes_iter`` and its root is a ``random.choice``; ``totals["reference_ran"]`` records
that as 0."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import components_utils as cu  # noqa: E402
import cyclic_utils as cy  # noqa: E402
import superbubble_utils as su  # noqa: E402
from test_partition_oracle import CASES as PARTITION_CASES, stage_inputs as partition_stage_inputs  # noqa: E402

SITUATIONS = ("rootless_first_root_certified", "rootless_two_or_more_runs", "cycle_exhausted_without_a_certificate",
              "three_or_more_split_levels", "edge_filter_fired", "split_node_as_entrance", "split_node_as_exit",
              "node_inside_from_a_later_run")


def application(edges, order, totals, extra):
    edges = [(int(e[0]), int(e[1])) for e in edges]
    order = [int(x) for x in order]
    sync = cy.scheme_all(edges, order)
    brute = cy.small_enough(edges, order)
    if brute:
        plain, parts = cy.definition_all(edges, order), cy.by_partition(edges, order)
        for k in cy.ARRAY_KEYS:
            assert np.array_equal(plain[k], parts[k]), "the partitions differ from the whole graph: " + k
            assert np.array_equal(plain[k], sync[k]), "the scheme differs from the definition: " + k
        for k in cy.STAT_KEYS:
            assert plain["stats"][k] == parts["stats"][k] == sync["stats"][k], k
    old = su.definition(edges, order) if len(order) <= su.BRUTE_FORCE_UP_TO else su.scheme(edges, order)
    cy.check_singleton_part(sync, old, edges, order)
    st, met = sync["stats"], sync["situations"]
    assert st["n_bubbles"] - st["n_cyclic_bubbles"] == old["stats"]["n_bubbles"]
    rec = cy.record_of(sync)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    rec["in_sha256"] = cu.digest(order, e[np.lexsort((e[:, 1], e[:, 0]))])
    rec.update(extra)
    rec["n_acyclic_bubbles"] = old["stats"]["n_bubbles"]
    rec["roots_of_first_rootless"] = [run[min(run)] for run in sync["roots_of_runs"] if run]
    totals["applications"] += 1
    totals["brute_forced"] += brute
    totals["with_a_cyclic_bubble"] += st["n_cyclic_bubbles"] > 0
    totals["cyclic_bubbles"] += st["n_cyclic_bubbles"]
    totals["digest_records"] += "sha256" in rec
    totals["rootless_first_root_certified"] += st["n_rootless"] > 0 and st["n_root_runs"] == 1 and st["n_certified"] == st["n_rootless"]
    totals["rootless_two_or_more_runs"] += st["n_rootless"] > 0 and st["n_root_runs"] >= 2
    totals["cycle_exhausted_without_a_certificate"] += st["n_certified"] < st["n_rootless"]
    totals["three_or_more_split_levels"] += st["n_split_levels"] >= 3
    totals["edge_filter_fired"] += st["n_edge_filtered"] > 0
    totals["split_node_as_entrance"] += met["split_entrance"] > 0
    totals["split_node_as_exit"] += met["split_exit"] > 0
    totals["node_inside_from_a_later_run"] += met["inside_from_a_later_run"] > 0
    return rec


def main():
    totals = {k: 0 for k in ("applications", "brute_forced", "with_a_cyclic_bubble", "cyclic_bubbles", "digest_records", "reference_ran") + SITUATIONS}
    cases = []
    for c in PARTITION_CASES:
        if c.get("direct"):
            continue
        stages = partition_stage_inputs(c)
        out = {"name": c["name"], "results": []}
        for stage in ("b", "c"):
            edges, order, n_ids = stages[stage]
            out["results"].append(application(cu.uv_of(edges).tolist(), order, totals, {"stage": stage, "n_ids": n_ids}))
        b, cc = out["results"]
        print("%-30s b: %5d nodes %4d bubbles (%d cyclic)  c: %5d / %4d (%d)" % (c["name"], b["n_nodes"], b["n_bubbles"], b["n_cyclic_bubbles"],
                                                                                cc["n_nodes"], cc["n_bubbles"], cc["n_cyclic_bubbles"]), flush=True)
        cases.append(out)
    for name, order, edges, n_ids in cy.direct_inputs():
        rec = application(edges, order, totals, {"stage": "a", "n_ids": n_ids if n_ids is not None else max(list(order) + [-2]) + 2})
        cases.append({"name": "direct_" + name, "direct": True, "host_only": n_ids is not None, "results": [rec]})
        print("%-58s nodes %5d  %5d bubbles (%d nested, %d cyclic)  split %d in %d levels, %d rootless, %d runs, %d certified, %d filtered" % (
            "direct_" + name, rec["n_nodes"], rec["n_bubbles"], rec["n_nested"], rec["n_cyclic_bubbles"], rec["n_split"], rec["n_split_levels"],
            rec["n_rootless"], rec["n_root_runs"], rec["n_certified"], rec["n_edge_filtered"]), flush=True)
    for k in SITUATIONS + ("brute_forced", "with_a_cyclic_bubble"):
        assert totals[k] > 0, "situation %s never occurs" % k
    cy.save_golden({"totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", cy.GOLDEN_FILE, len(cases), "cases", os.path.getsize(cy.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
