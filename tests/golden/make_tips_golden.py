#!/usr/bin/env python3
"""Generate tests/golden/tips_cases.npz by EXECUTING the reference's own functions.

Runs only where the reference checkout is present (/root/reference); the output is committed.  Every case goes through
what `phasm layout` does at phasm/cli/assembler.py:161-167 (and, for some, again as at :177-179):

    phasm.assembly_graph.remove_incoming_tips(g, L, B)    -> flag 1
    phasm.assembly_graph.remove_outgoing_tips(g, L, B)    -> flag 2
    phasm.assembly_graph.make_symmetric(g)                -> flag 3
    phasm.assembly_graph.clean_graph(g)                   -> isolated nodes, the node order left

on a graph that make_reduce_golden.stage1_graph built (the reference's build_assembly_graph on GFA2 text), reduced first
where the case says so, or -- the "direct" cases -- on a graph filled edge by edge, which reaches weights <= 0 (stage 1
never emits them) and self-loops, 2-cycles and the edge (a, a^1) (which no text case here brings).  The functions are imported and run unmodified on ``TipsGraph``: the
stand-in of make_reduce_golden plus the networkx 1.x calls these four make (``in_degree``, list-valued ``predecessors``
and ``neighbors``, ``nodes_iter``, ``remove_nodes_from``) and the reference's own ``path_length``, borrowed from its
AssemblyGraph class.  ``node_path_edges`` is a stand-in with the same contract: the reference's generator ends by letting
``next()`` raise StopIteration inside the generator, which Python >= 3.7 turns into a RuntimeError (PEP 479).

Branch totals come from tests/tips_utils.py, whose flags, counts and node order must equal the reference's on every case
here (asserted below, sequential statement and round scheme alike)."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import phasm.assembly_graph as ag  # noqa: E402  (reference)

RefAssemblyGraph = ag.AssemblyGraph    # (make_reduce_golden points the module's name at its stand-in)

import make_reduce_golden as mrg  # noqa: E402
import reduce_utils as ru  # noqa: E402
import tips_utils as tu  # noqa: E402
from phasm_amd.io import gfa as pgfa  # noqa: E402


class TipsGraph(mrg.StandInGraph):
    path_length = RefAssemblyGraph.path_length

    def in_degree(self, n):
        return len(self.pred[n])

    def predecessors(self, n):
        return list(self.pred[n])

    def neighbors(self, n):
        return list(self.adj[n])

    def nodes_iter(self):
        return iter(self.adj)

    def remove_nodes_from(self, nodes):
        for n in list(nodes):
            if n in self.adj:
                self.remove_node(n)

    def node_path_edges(self, nodes, data=None):
        """What the two tip functions need of it: the consecutive pairs of ``nodes`` as (u, v), or as (u, v, x) with x
        the edge's attribute dict (``data is True``) or one attribute of it (``data`` = its name).  A pair that is no
        edge is a KeyError."""
        pairs = list(zip(nodes, nodes[1:]))
        if not data:
            return iter(pairs)
        pick = (lambda attrs: attrs) if data is True else (lambda attrs: attrs[data])
        return ((u, v, pick(self.adj[u][v])) for u, v in pairs)


ag.AssemblyGraph = TipsGraph
SMALL = 30000          # stage-1 edges: the cases of reduce_cases.npz below this size ...
ALSO = ("cfg2_1k",)    # ... and this one
TWICE = ("cfg2_1k", "tie_8", "line_100", "line_105", "line_108", "line_111", "tangle", "junction", "comb_4", "direct", "selfish")


class N(int):
    """A node of a direct case: an oriented-read index with the one method make_symmetric calls."""

    def reverse(self):
        return N(int(self) ^ 1)


def edge_set(g, idx):
    return {(idx(u), idx(v)) for u, v in g.edges_iter()}


def run_tips(g, idx, L, B, totals, second):
    """The four calls on g (changed in place).  Returns the record of this application."""
    order = [idx(n) for n in g]
    e_in = np.asarray([[idx(u), idx(v), int(d[g.edge_len]), int(d.get(g.overlap_len, 0))] for u, v, d in g.edges_iter(data=True)],
                      dtype=np.int64).reshape(-1, 4)
    n_in = ag.remove_incoming_tips(g, L, B)
    after_in = edge_set(g, idx)
    n_out = ag.remove_outgoing_tips(g, L, B)
    after_out = edge_set(g, idx)
    n_asym = ag.make_symmetric(g)
    kept = edge_set(g, idx)
    n_iso = ag.clean_graph(g)
    left = [idx(n) for n in g]
    flags = np.array([0 if uv in kept else 3 if uv in after_out else 2 if uv in after_in else 1
                      for uv in map(tuple, e_in[:, :2].tolist())], dtype=np.uint8)
    assert (n_in, n_out, n_asym) == tuple(int((flags == f).sum()) for f in (1, 2, 3)), "a path named an edge twice"
    # the restatement and the round scheme on the same input
    counts = tu.new_counts()
    mine, mine_left, st = tu.remove_tips(e_in, order, L, B, counts)
    assert np.array_equal(mine, flags) and mine_left == left and st["n_isolated_nodes"] == n_iso, "restatement differs"
    for seed in (1, 2):
        rf, r_in, r_out = tu.remove_tips_rounds(e_in, order, L, B, seed)
        assert np.array_equal(rf, np.where(flags == 3, 0, flags)), "round scheme differs"
        totals["max_rounds"] = max(totals["max_rounds"], r_in, r_out)
    rev, _, _ = tu.remove_tips(e_in, order[::-1], L, B)
    sensitive = not np.array_equal(rev, flags)
    if not second:
        for k, v in counts.items():
            totals[k] += v
        totals["order_sensitive_cases"] += sensitive
    o = tu.by_uv(e_in)
    return {"L": L, "B": B, "n_in": len(e_in), "n_in_tip_edges": int(n_in), "n_out_tip_edges": int(n_out),
            "n_asymmetric": int(n_asym), "n_isolated_nodes": int(n_iso), "n_kept": len(kept), "n_nodes": len(order),
            "n_candidates_in": st["n_candidates_in"], "n_candidates_out": st["n_candidates_out"],
            "order_sensitive": bool(sensitive), "flags": ru.pack_flags(flags[o]),
            "kept_sha256": ru.edge_digest(e_in[o][flags[o] == 0]), "order_left": left}, order


def twice(name):
    return any(name.startswith(t) for t in TWICE)


def text_case(name, source, params, fuzzes, LB, totals):
    text = tu.case_text(source)
    out = dict(source, name=name, params=params, results=[])
    for fuzz in fuzzes:
        for L, B in LB:
            g, node_index = mrg.stage1_graph(text, params)
            idx = lambda n: node_index[str(n)]   # noqa: E731
            order = [idx(n) for n in g]
            if fuzz is not None:
                g.remove_edges_from(ag.remove_transitive_edges(g, fuzz))
                ag.make_symmetric(g)
            rec, order2 = run_tips(g, idx, L, B, totals, False)
            assert order2 == order                      # the reduction removes no node
            rec["fuzz"] = fuzz
            if twice(name):
                rec2, _ = run_tips(g, idx, L, tu.DEFAULT_B, totals, True)
                rec.update({"flags2": rec2["flags"], "order_left2": rec2["order_left"],
                            "second": {k: rec2[k] for k in rec2 if k not in ("flags", "order_left")}})
            out["results"].append(rec)
    # the node-order rule on the rows the device will read
    names, lengths, rows = pgfa.read_gfa2_rows(text.splitlines(True))
    assert tu.node_order(rows.tolist(), np.repeat(lengths, 2).tolist(), **params) == order, name
    out["order"] = order
    print("%-30s nodes %6d  " % (name, len(order)) + "  ".join(
        "F%s L%d B%d: %d/%d/%d/%d" % (r["fuzz"], r["L"], r["B"], r["n_in_tip_edges"], r["n_out_tip_edges"], r["n_asymmetric"],
                                       r["n_isolated_nodes"]) for r in out["results"]))
    return out


def direct_graph(seed):
    """A random small graph with weights of either sign, twins for most edges, a few nodes without edges, and -- every
    third seed -- a self-loop, a 2-cycle and an edge (a, a^1); nodes enter in a random order."""
    rng = random.Random(seed)
    n_reads = rng.randrange(8, 20)
    nodes = list(range(2 * n_reads))
    edges = {}
    for _ in range(rng.randrange(n_reads, 3 * n_reads)):
        u, v = rng.sample(nodes, 2)
        if rng.random() < 0.7:                          # chains: low degrees, where tips live
            if any(a == u for a, _ in edges) or any(b == v for _, b in edges):
                continue
        w = rng.choice([-700, -1, 0, 1, 400, 1200, 2499, 2500, 2501, 5000, 5001])
        edges[(u, v)] = w
        if rng.random() < 0.85:
            edges.setdefault((v ^ 1, u ^ 1), rng.choice([w, w, 300]))
    if seed % 3 == 0:
        a, b, c = rng.sample(range(n_reads), 3)
        edges[(2 * a, 2 * a)] = 10
        edges[(2 * b, 2 * b + 1)] = 20
        edges[(2 * c, 2 * a + 1)] = 5
        edges[(2 * a + 1, 2 * c)] = 5
    items = list(edges.items())
    rng.shuffle(items)
    order = [n for n in nodes if rng.random() < 0.9]
    rng.shuffle(order)
    return order, [(u, v, w) for (u, v), w in items]


def direct_case(name, order, edges, LB, totals):
    out = {"name": name, "direct": True, "results": []}
    first = None
    for L, B in LB:
        g = TipsGraph(edge_len="weight", overlap_len="overlap_len")
        for n in order:
            g._node(N(n))
        for u, v, w in edges:
            g.add_edge(N(u), N(v), {"weight": w, "overlap_len": 0})
        e_all = [[int(u), int(v), int(d["weight"]), 0] for u, v, d in g.edges_iter(data=True)]
        rec, order_in = run_tips(g, int, L, B, totals, False)
        rec["fuzz"] = None
        rec2, _ = run_tips(g, int, L, tu.DEFAULT_B, totals, True)
        rec.update({"flags2": rec2["flags"], "order_left2": rec2["order_left"],
                    "second": {k: rec2[k] for k in rec2 if k not in ("flags", "order_left")}})
        out["results"].append(rec)
        first = first or (order_in, e_all)
    out["order"], out["edges"] = first
    print("%-30s nodes %6d  " % (name, len(out["order"])) + "  ".join(
        "L%d B%d: %d/%d/%d/%d" % (r["L"], r["B"], r["n_in_tip_edges"], r["n_out_tip_edges"], r["n_asymmetric"], r["n_isolated_nodes"])
        for r in out["results"]))
    return out


def main():
    totals = dict(tu.new_counts(), max_rounds=0)
    default = ru.DEFAULT_PARAMS
    std = [(tu.DEFAULT_L, tu.DEFAULT_B)]
    cases = []
    for c in ru.load_golden()["cases"]:
        if c["n_stage1"] >= SMALL and c["name"] not in ALSO:
            continue
        fuzzes = [int(f) for f in c["results"]]
        cases.append(text_case("reduced_" + c["name"], {"reduce_case": c["name"]}, c["params"], fuzzes, std, totals))

    def synth(name, kw, fuzzes, LB):
        src = {"synth": kw}
        src["text_sha256"] = ru.text_digest(tu.case_text(src))
        cases.append(text_case(name, src, default, fuzzes, LB, totals))

    for order in tu.JUNCTION_ORDERS:                    # tips straight from the stage-1 result
        synth("junction_" + order, {"kind": "junction", "order": order}, [None], std)
    for L in (0, 1, 4):
        synth("comb_%d" % L, {"kind": "comb", "L": L}, [None, 1000], [(L, tu.DEFAULT_B)])
    seed, found = 0, 0
    while found < 10:
        seed += 1
        before = dict(totals)
        scratch = dict(tu.new_counts(), max_rounds=0)
        probe = text_case("tangle_%d" % seed, {"synth": {"kind": "tangle", "seed": seed}}, default, [None], std, scratch)
        r = probe["results"][0]
        # keep the seeds that bring something: a walk through an emptied junction, an order-sensitive answer, or asymmetry
        if not (scratch["through_emptied_junction"] and (r["order_sensitive"] or r["n_asymmetric"])):
            continue
        assert totals == before
        synth("tangle_%d" % seed, {"kind": "tangle", "seed": seed}, [None, 0], std + [(2, 2500)])
        found += 1
    # reads aligned with themselves and with their own reverse strand: self-loops, (a, a^1), 2-cycles from GFA text
    for seed in (1, 2, 3):
        synth("selfish_%d" % seed, {"kind": "selfish", "seed": seed}, [None, 0], std + [(2, 2500)])
    for seed in range(1, 19):
        order, edges = direct_graph(seed)
        cases.append(direct_case("direct_%d" % seed, order, edges, std + [(1, 2500), (0, 5000), (7, 100000)], totals))
    for k, v in totals.items():
        assert v > 0, "branch %s never taken" % k
    tu.save_golden({"branch_totals": totals, "cases": cases})
    print("totals", totals)
    print("wrote", tu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(tu.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
