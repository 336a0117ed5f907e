#!/usr/bin/env python3
"""Generate tests/golden/diamond_cases.npz by EXECUTING the reference's own functions.

Runs only where the reference checkout is present (/root/reference); the output is committed.

    phasm.assembly_graph.remove_diamond_tips(g)           phasm/assembly_graph.py:721-743, assembler.py:173

runs unmodified on the stand-in graph of make_tips_golden plus ``predecessors_iter``:
  (a) on the stage-1 graph of every text case of tips_cases.npz,
  (b) on that graph after the reduction at fuzz 1000 and the first tip block at (4, 5000),
  and on direct cases filled edge by edge, whose nodes have a positive ``__len__`` (the reference tests the truth value
  of a node, :736; an OrientedRead is true iff it has a length).
(b) is one step of the WHOLE chain of `phasm layout` stage 2 up to the merging of paths (assembler.py:145-182) at the CLI
defaults, which is recorded per text case too: what removed every stage-1 edge (``removed_by``), the digest of the edges
left, the node order left and the counts the command logs.

Branch totals come from tests/diamond_utils.py, whose flags, counts and node order must equal the reference's on every
application here (asserted below, sequential statement and round scheme alike)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_tips_golden as mtg  # noqa: E402  (sets the paths up; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)

import diamond_utils as du  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import reduce_utils as ru  # noqa: E402
import tips_utils as tu  # noqa: E402


class DiamondGraph(mtg.TipsGraph):
    def predecessors_iter(self, n):
        return iter(list(self.pred[n]))


ag.AssemblyGraph = DiamondGraph


class M(int):
    """A node of a direct case: an oriented-read index that is true whatever its index, like a read with a length."""

    def __len__(self):
        return 1

    def __bool__(self):
        return len(self) > 0

    def reverse(self):
        return M(int(self) ^ 1)


def edge_array(g, idx):
    return np.asarray([[idx(u), idx(v), int(d[g.edge_len]), int(d.get(g.overlap_len, 0))] for u, v, d in g.edges_iter(data=True)],
                      dtype=np.int64).reshape(-1, 4)


def edge_set(g, idx):
    return {(idx(u), idx(v)) for u, v in g.edges_iter()}


def run_diamonds(g, idx, stage, totals, case_order):
    """remove_diamond_tips on g (changed in place).  Returns the record of this application and its flags in graph order."""
    order = [idx(n) for n in g]
    e_in = edge_array(g, idx)
    out0 = {}
    for u, _v in e_in[:, :2].tolist():
        out0[u] = out0.get(u, 0) + 1
    n_diamonds = ag.remove_diamond_tips(g)
    kept = edge_set(g, idx)
    left = [idx(n) for n in g]
    gone_nodes = set(order) - set(left)
    assert left == [n for n in order if n not in gone_nodes] and len(gone_nodes) == 2 * n_diamonds
    # an edge that left went into a removed node: an end node (no out-edge at the start) or a pred1
    flags = np.zeros(len(e_in), dtype=np.uint8)
    for k, (u, v) in enumerate(e_in[:, :2].tolist()):
        if (u, v) not in kept:
            assert v in gone_nodes
            flags[k] = 1 if out0.get(v, 0) == 0 else 2
    assert int((flags != 0).sum()) == 3 * n_diamonds and int((flags == 2).sum()) == n_diamonds
    counts = du.new_counts()
    mine, mine_left, st = du.remove_diamond_tips(e_in, order, counts)
    assert np.array_equal(mine, flags) and mine_left == left and st["n_diamonds"] == n_diamonds, "restatement differs"
    rounds = 0
    for seed in (1, 2, 3):
        rf, r = du.remove_diamond_tips_rounds(e_in, order, seed)
        assert np.array_equal(rf, flags), "round scheme differs"
        rounds = max(rounds, r)
    rev, _, _ = du.remove_diamond_tips(e_in, order[::-1])
    sensitive = not np.array_equal(rev, flags)
    for k, v in counts.items():
        totals[k] += v
    totals["order_sensitive_cases"] += sensitive
    totals["max_rounds"] = max(totals["max_rounds"], rounds)
    o = tu.by_uv(e_in)
    before = set(order)
    rec = {"stage": stage, "n_in": len(e_in), "n_kept": len(kept), "n_nodes": len(order), "n_candidates": st["n_candidates"],
           "n_diamonds": int(n_diamonds), "rounds": rounds, "order_sensitive": bool(sensitive), "flags": ru.pack_flags(flags[o]),
           "kept_sha256": ru.edge_digest(e_in[o][flags[o] == 0]),
           "gone_before": [n for n in case_order if n not in before], "gone": [n for n in order if n in gone_nodes]}
    assert du.minus(case_order, rec["gone_before"]) == order
    return rec, flags


def text_case(c, totals):
    name, params = c["name"], c["params"]
    text = du.case_text(c)
    out = {k: c[k] for k in ("reduce_case", "synth", "text_sha256") if k in c}
    out.update(name=name, params=params, results=[])
    # (a) the stage-1 graph
    g, node_index = mrg.stage1_graph(text, params)
    idx = lambda n: node_index[str(n)]   # noqa: E731
    order = [idx(n) for n in g]
    assert order == c.get("order", order)
    for n in g:
        assert len(n) > 0                # the truth value the reference tests, assembly_graph.py:736
    rec, _ = run_diamonds(g, idx, "a", totals, order)
    out["results"].append(rec)
    # the chain, assembler.py:145-182, with (b) as its third step
    g, node_index = mrg.stage1_graph(text, params)
    s1 = edge_array(g, idx)
    uv = [tuple(x) for x in s1[:, :2].tolist()]
    removed_by = np.zeros(len(s1), dtype=np.uint8)

    def note(code):
        live = edge_set(g, idx)
        for k, e in enumerate(uv):
            if removed_by[k] == 0 and e not in live:
                removed_by[k] = code

    transitive = ag.remove_transitive_edges(g, du.STAGE_FUZZ)
    n_transitive = len(transitive)
    g.remove_edges_from(transitive)
    note(1)
    n_asym = ag.make_symmetric(g)
    note(2)
    n_in = ag.remove_incoming_tips(g, du.STAGE_L, du.STAGE_B)
    note(3)
    n_out = ag.remove_outgoing_tips(g, du.STAGE_L, du.STAGE_B)
    note(4)
    n_asym += ag.make_symmetric(g)
    note(5)
    n_iso = ag.clean_graph(g)
    e_b = edge_array(g, idx)
    rec, flags = run_diamonds(g, idx, "b", totals, order)
    out["results"].append(rec)
    # (by pair: the reduction has sorted the adjacency lists, so the graph no longer lists its edges in the order of s1)
    by_pair = {tuple(e_b[k, :2].tolist()): int(f) for k, f in enumerate(flags)}
    for k, e in enumerate(uv):
        if removed_by[k] == 0 and by_pair.get(e, 0):
            removed_by[k] = 5 + by_pair[e]
    n_in2 = ag.remove_incoming_tips(g, du.STAGE_L)      # (remove_tips(g, L): the base bound is the function's default)
    note(8)
    n_out2 = ag.remove_outgoing_tips(g, du.STAGE_L)
    note(9)
    n_asym2 = ag.make_symmetric(g)
    note(10)
    n_iso2 = ag.clean_graph(g)
    left = [idx(n) for n in g]
    final = edge_array(g, idx)
    o = tu.by_uv(s1)
    reduce_flags = np.where(removed_by <= 2, removed_by, 0)
    mine, mine_e, mine_left, stats = du.clean_chain(s1, order, reduce_flags=reduce_flags)
    counts = {"n_transitive": n_transitive, "n_asymmetric": int(n_asym), "n_tip_edges": int(n_in + n_out), "n_isolated_nodes": int(n_iso),
              "n_diamonds": rec["n_diamonds"], "n_tip_edges2": int(n_in2 + n_out2), "n_isolated_nodes2": int(n_iso2),
              "n_asymmetric2": int(n_asym2)}
    assert np.array_equal(mine, removed_by) and mine_left == left and du.chain_counts(stats) == counts, "the restated chain differs"
    assert ru.sort_edges(mine_e).tolist() == ru.sort_edges(final).tolist()
    totals["asymmetric_second_tips"] += int(n_asym2)
    totals["chains_with_every_code"] += set(range(1, 11)) <= set(removed_by.tolist())
    for code in range(1, 11):
        totals["code_%d" % code] += int((removed_by == code).sum())
    out["chain"] = dict(counts, n_stage1=len(s1), n_kept=len(final), kept_sha256=ru.edge_digest(ru.sort_edges(final)),
                        fuzz=du.STAGE_FUZZ, L=du.STAGE_L, B=du.STAGE_B)
    out["removed_by"] = removed_by[o].tolist()
    gone = set(order) - set(left)
    out["chain_gone"] = [n for n in order if n in gone]
    out["order_full"] = order
    print("%-30s nodes %6d  a: %d/%d  b: %d/%d (%d rounds)  chain: %s" % (
        name, len(order), out["results"][0]["n_diamonds"], out["results"][0]["n_candidates"], rec["n_diamonds"], rec["n_candidates"],
        rec["rounds"], " ".join(str(int((removed_by == k).sum())) for k in range(11))))
    return out


# ---- direct cases --------------------------------------------------------------------------------------------------

def fan(K, last="pred1"):
    """K end nodes on one hub G (W -> G), each with a private chain S_i -> P_i -> E_i.  The diamonds take G's out-edges
    one by one, in node order: every end node shares G, so the device settles one per round.  ``last``: what the last end
    node has beside G -- "pred1" its chain like the others (G's out-degree is 1 by then: no gt1 left), "gt1" a node R
    with a second out-edge (G, in-degree 1, has become pred1 and goes), "none" nothing (in-degree 1: no candidate)."""
    W, G = 0, 2
    edges, nxt = [(W, G)], 4
    for i in range(K):
        S, P, E = nxt, nxt + 2, nxt + 4
        nxt += 6
        edges.append((G, E))
        if i < K - 1 or last == "pred1":
            edges += [(S, P), (P, E)]
        elif last == "gt1":
            edges += [(S, E), (S, P)]
    return edges


def direct_inputs():
    Z, Q, E1, E2, X, P, R, Y = 0, 2, 4, 6, 8, 10, 12, 14
    q = [(Z, Q), (Q, E1), (Q, E2), (X, P), (P, E1), (R, E2), (R, Y)]
    cases = [("q_e1_first", [Z, Q, E1, E2, X, P, R, Y], q), ("q_e2_first", [Z, Q, E2, E1, X, P, R, Y], q)]
    for K in (2, 3, 64, 65):
        cases.append(("fan_%d" % K, None, fan(K)))
    cases.append(("fan_3_last_gt1", None, fan(3, "gt1")))
    cases.append(("fan_65_last_gt1", None, fan(65, "gt1")))
    cases.append(("fan_3_last_none", None, fan(3, "none")))
    cases.append(("pp_is_gt1", None, [(0, 2), (2, 4), (2, 6), (4, 6)]))                       # W -> G, G -> P, G -> E, P -> E
    cases.append(("pp_is_gt1_node0_pred1", [6, 0, 2, 4], [(6, 2), (2, 0), (2, 4), (0, 4)]))  # the same with pred1 = node 0
    cases.append(("both_pred1", None, [(0, 2), (2, 8), (4, 6), (6, 8)]))
    cases.append(("both_gt1", None, [(0, 8), (0, 2), (4, 8), (4, 6)]))
    cases.append(("pred1_in0", None, [(0, 8), (4, 8), (4, 6)]))
    cases.append(("pred1_in2", None, [(0, 4), (2, 4), (4, 8), (6, 8), (6, 10)]))
    cases.append(("gt1_self_loop", None, [(0, 0), (0, 8), (2, 4), (4, 8)]))
    cases.append(("pp_two_cycle", None, [(0, 2), (2, 0), (2, 4), (4, 8), (6, 8), (6, 10)]))
    cases.append(("pred_is_mirror", None, [(9, 8), (9, 2), (4, 6), (6, 8)]))                 # E = 8, gt1 = E^1 = 9
    cases.append(("pred1_is_mirror", None, [(2, 9), (9, 8), (4, 8), (4, 6)]))                # pred1 = E^1
    cases.append(("empty", [], []))
    cases.append(("nodes_without_edges", [4, 2, 0], []))
    cases.append(("no_candidates", None, [(2 * i, 2 * i + 2) for i in range(9)]))
    # several of the above in one graph, shifted apart, candidates interleaved in the node order
    big, order = [], []
    for j, (_, o, e) in enumerate([c for c in cases if c[0] in ("q_e1_first", "q_e2_first", "fan_3", "pp_is_gt1", "pp_two_cycle")]):
        off = 200 * j
        big += [(u + off, v + off) for u, v in e]
        order.append([n + off for n in (o if o is not None else first_seen(e))])
    mixed = [row[i] for i in range(max(map(len, order))) for row in order if i < len(row)]
    cases.append(("mixed", mixed, big))
    return cases


def first_seen(edges):
    seen = []
    for u, v in edges:
        for n in (u, v):
            if n not in seen:
                seen.append(n)
    return seen


def direct_case(name, order, edges, totals):
    g = DiamondGraph(edge_len="weight", overlap_len="overlap_len")
    for n in (order if order is not None else []):
        g._node(M(n))
    for u, v in edges:
        g.add_edge(M(u), M(v), {"weight": 500, "overlap_len": 0})
    case_order = [int(n) for n in g]
    e_all = edge_array(g, int).tolist()
    rec, _ = run_diamonds(g, int, "a", totals, case_order)
    print("%-30s nodes %6d  %d/%d (%d rounds)" % ("direct_" + name, len(case_order), rec["n_diamonds"], rec["n_candidates"], rec["rounds"]))
    return {"name": "direct_" + name, "direct": True, "results": [rec], "order": case_order, "edges": e_all}


def main():
    totals = dict(du.new_counts(), max_rounds=0, **{"code_%d" % k: 0 for k in range(1, 11)})
    cases = []
    tips = tu.load_golden()
    for c in tips["cases"]:
        if not c.get("direct"):
            cases.append(text_case(c, totals))
            del cases[-1]["order_full"]  # (tips_cases.npz holds it)
    # every step of the chain at work in ONE graph: no case of tips_cases.npz has that, so the first union of a tangle and
    # a line (tests/diamond_utils.py union_case) in which every code from 1 to 10 occurs joins the text cases
    for line in range(1, 400):
        src = {"name": "union_21_%d" % line, "params": ru.DEFAULT_PARAMS, "synth": {"kind": "union", "tangle": 21, "line": line}}
        src["text_sha256"] = ru.text_digest(du.case_text(src))
        scratch = dict(totals)
        probe = text_case(src, scratch)
        if scratch["chains_with_every_code"]:
            probe["order"] = probe.pop("order_full")
            cases.append(probe)
            totals.update(scratch)
            break
    text_totals = dict(totals)
    for name, order, edges in direct_inputs():
        cases.append(direct_case(name, order, edges, totals))
    for k in du.BRANCHES + ("max_rounds",):
        assert totals[k] > 0, "branch %s never taken" % k
    du.save_golden({"branch_totals": totals, "text_totals": text_totals, "cases": cases})
    print("totals", totals)
    print("wrote", du.GOLDEN_FILE, len(cases), "cases", os.path.getsize(du.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
