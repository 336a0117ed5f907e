#!/usr/bin/env python3
"""Generate tests/golden/merge_cases.npz by EXECUTING the reference's own functions.

Runs only where the reference checkout is present (/root/reference); the output is committed.

    phasm.assembly_graph.merge_unambiguous_paths(g)       phasm/assembly_graph.py:456-541, assembler.py:184-186
    phasm.io.gfa.gfa2_write_graph(f, g)                   phasm/io/gfa.py:281-326, assembler.py:195-212

run unmodified on the stand-in graph of make_diamond_golden plus ``add_node``, ``node``, ``in_edges_iter`` and
``out_edges_iter``:
  (a) on the stage-1 graph of every text case of tips_cases.npz, of the union case of diamond_cases.npz and of the ring and
      lasso cases of tests/merge_utils.py,
  (b) on that graph after the whole cleaning chain of assembler.py:145-182 at the CLI defaults, where the file the command
      writes is recorded too (digest of its H / S / F lines in order and of its sorted E lines),
  and on direct cases filled edge by edge, every node order given.

Branch totals come from tests/merge_utils.py, whose flags, tables, edges, node order and count must equal the reference's
on every application here (asserted below, the plain statement and the device's scheme alike).

    --time    also print what the reference's merge_unambiguous_paths takes on every stage-(b) graph, on this host core"""
import io
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_diamond_golden as mdg  # noqa: E402  (sets the paths up; the reference is importable after it)
import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads  # noqa: E402  (reference)

import diamond_utils as du  # noqa: E402
import make_reduce_golden as mrg  # noqa: E402
import merge_utils as mu  # noqa: E402
import reduce_utils as ru  # noqa: E402
import tips_utils as tu  # noqa: E402

TIME = "--time" in sys.argv


class MergeGraph(mdg.DiamondGraph):
    def __init__(self, data=None, **attr):
        super().__init__(data, **attr)
        self.node = {}

    def _node(self, n):
        super()._node(n)
        self.node.setdefault(n, {})

    def add_node(self, n):
        self._node(n)

    def remove_node(self, n):
        super().remove_node(n)
        self.node.pop(n, None)

    def in_edges_iter(self, n, data=False):
        for u, d in list(self.pred[n].items()):
            yield (u, n, d) if data else (u, n)

    def out_edges_iter(self, n, data=False):
        for v, d in list(self.adj[n].items()):
            yield (n, v, d) if data else (n, v)


ag.AssemblyGraph = MergeGraph


class P(mdg.M):
    """A node of a direct case: an oriented-read index with the length tests/merge_utils.py gives it."""

    id = property(lambda self: str(int(self)))   # (the reference's debug line names the nodes of a path)

    def __len__(self):
        return mu.direct_length(self)

    def reverse(self):
        return P(int(self) ^ 1)


def run_merge(g, idx0, n_ids, lengths, stage, totals, case_order, write=False):
    """merge_unambiguous_paths on g (changed in place).  Returns the record of this application."""
    order = [idx0(n) for n in g]
    e_in = mdg.edge_array(g, idx0)
    t0 = time.perf_counter()
    n_merged_nodes = ag.merge_unambiguous_paths(g)
    seconds = time.perf_counter() - t0
    merged = [n for n in g if isinstance(n, MergedReads)]
    assert [n.id for n in merged] == ["merged%d" % k for k in range(len(merged))] and all(n.strand == "+" for n in merged)
    k_of = {str(n): k for k, n in enumerate(merged)}

    def idx(n):
        return n_ids + k_of[str(n)] if isinstance(n, MergedReads) else idx0(n)

    members, prefix, path_nodes, plen, links, on_path = [], [], [], [], set(), set()
    for n in merged:
        reads = [idx0(r) for r in n.reads]
        assert len(n.prefix_lengths) == len(reads) - 1 >= 1
        members += reads
        prefix += [int(x) for x in n.prefix_lengths] + [0]
        path_nodes.append(len(reads))
        plen.append(len(n))
        links.update(zip(reads, reads[1:]))
        on_path.update(reads)
    assert n_merged_nodes == len(members) == len(on_path)
    left = [idx(n) for n in g]
    assert left == [n for n in order if n not in on_path] + [n_ids + k for k in range(len(merged))]
    flags = np.array([1 if (u, v) in links else 2 if (u in on_path or v in on_path) else 0 for u, v in e_in[:, :2].tolist()],
                     dtype=np.uint8)
    e_out = mdg.edge_array(g, idx)
    assert len(e_out) == len(e_in) - (len(members) - len(merged)) == int((flags != 1).sum())
    # the restatement and the device's scheme on the same input
    counts = mu.new_counts()
    mine = mu.merge_paths(e_in, order, lengths, n_ids, counts)
    want = {"flags": flags, "members": np.asarray(members, np.int64), "prefix": np.asarray(prefix, np.int64),
            "lengths": np.asarray(plen, np.int64), "offsets": np.concatenate([[0], np.cumsum(path_nodes)]).astype(np.int64)}
    rounds = 0
    for res in [mine] + [mu.merge_paths_rounds(e_in, order, lengths, n_ids, seed) for seed in (1, 2)]:
        for key, w in want.items():
            assert np.array_equal(res[key], w), "restatement differs: " + key
        assert res["order"] == left and res["stats"]["n_nodes_merged"] == n_merged_nodes
        assert ru.sort_edges(res["edges"]).tolist() == ru.sort_edges(e_out).tolist(), "restatement differs: edges"
        rounds = max(rounds, res["stats"]["n_rounds"] or 0)
    for k, v in counts.items():
        totals[k] += v
    totals["max_rounds"] = max(totals["max_rounds"], rounds)
    totals["applications"] += 1
    o = tu.by_uv(e_in)
    before = set(order)
    rec = {"stage": stage, "n_in": len(e_in), "n_ids": n_ids, "rounds": rounds, "flags": ru.pack_flags(flags[o]),
           "kept_sha256": ru.edge_digest(ru.sort_edges(e_out)), "gone_before": [n for n in case_order if n not in before],
           "members": members, "prefix": prefix, "path_nodes": path_nodes, "lengths": plen}
    rec.update({k: mine["stats"][k] for k in mu.STAT_KEYS})
    assert du.minus(case_order, rec["gone_before"]) == order
    if write:
        f = io.StringIO()
        rgfa.gfa2_write_graph(f, g)
        lines = f.getvalue().splitlines(True)
        head, e_lines = [l for l in lines if l[0] != "E"], [l for l in lines if l[0] == "E"]
        assert lines == head + e_lines
        rec["hsf_sha256"], rec["e_sorted_sha256"] = mu.lines_digest(head), mu.lines_digest(sorted(e_lines))
        rec["n_hsf_lines"] = len(head)
        names = {i: s for s, i in write.items()}
        my_head, my_e = mu.gfa_lines(mine, names, lengths, n_ids)
        assert my_head == head and sorted(my_e) == sorted(e_lines), "the restated file differs"
    return rec, seconds


def text_case(c, totals, own_order=False):
    name, params = c["name"], c["params"]
    text = mu.case_text(c)
    out = {k: c[k] for k in ("reduce_case", "synth", "text_sha256") if k in c}
    out.update(name=name, params=params, results=[])
    g, node_index = mrg.stage1_graph(text, params)
    idx = lambda n: node_index[str(n)]   # noqa: E731
    n_ids = len(node_index)
    lengths = np.zeros(n_ids, dtype=np.int64)
    for n in g:
        lengths[idx(n)] = len(n)
    order = [idx(n) for n in g]
    assert order == c.get("order", order)
    rec, _ = run_merge(g, idx, n_ids, lengths, "a", totals, order)
    out["results"].append(rec)
    # the chain, assembler.py:145-182, then (b)
    g, node_index = mrg.stage1_graph(text, params)
    g.remove_edges_from(ag.remove_transitive_edges(g, du.STAGE_FUZZ))
    ag.make_symmetric(g)
    ag.remove_tips(g, du.STAGE_L, du.STAGE_B)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    ag.remove_diamond_tips(g)
    ag.remove_tips(g, du.STAGE_L)
    ag.make_symmetric(g)
    ag.clean_graph(g)
    if "chain_order_left" in c:
        assert [idx(n) for n in g] == c["chain_order_left"], "the chain differs from diamond_cases.npz"
    rec, seconds = run_merge(g, idx, n_ids, lengths, "b", totals, order, write=node_index)
    out["results"].append(rec)
    if own_order:
        out["order"] = order
    print("%-30s nodes %6d  a: %d paths / %d nodes  b: %d / %d (longest %d, %d rounds, %d self-loops, %d on cycles)%s" % (
        name, len(order), out["results"][0]["n_merged"], out["results"][0]["n_nodes_merged"], rec["n_merged"], rec["n_nodes_merged"],
        rec["max_path_nodes"], rec["rounds"], rec["n_self_loops"], rec["n_cycle_nodes"],
        "  reference: %.3f ms" % (1e3 * seconds) if TIME else ""))
    return out


# ---- direct cases --------------------------------------------------------------------------------------------------

def chain(nodes, w0=100):
    return [(a, b, w0 + 7 * i % 50) for i, (a, b) in enumerate(zip(nodes, nodes[1:]))]


def direct_inputs():
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    cases = []
    for n in (2, 3, 64):
        cases.append(("path_%d" % n, ev(n), chain(ev(n))))
    scr = ev(65)
    random.Random(65).shuffle(scr)
    cases.append(("path_65_scrambled", scr, chain(ev(65))))
    for n in (1025, 4097):
        cases.append(("path_%d_reversed" % n, ev(n)[::-1], chain(ev(n))))
    for n in (1, 2, 3, 64, 65):
        ring = ev(n)
        cases.append(("cycle_%d" % n, ring, chain(ring + ring[:1])))
    ring, tail = ev(6), ev(2, 20)
    lasso = chain(ring + ring[:1]) + chain(tail + ring[:1], 300)
    cases.append(("lasso_tail_first", tail + ring, lasso))
    cases.append(("lasso_ring_reversed_first", ring[::-1] + tail, lasso))
    other = ev(3, 40)
    cases.append(("lasso_exit_into_a_path", other[::-1] + ring + tail, lasso + [(ring[-1], other[0], 77)] + chain(other, 500)))
    cases.append(("two_cycle_with_tail", [0, 2, 4], [(0, 2, 110), (2, 0, 120), (4, 0, 130)]))
    cases.append(("path_into_self_loop", [4, 2, 0], [(0, 2, 110), (2, 4, 120), (4, 4, 130)]))
    cases.append(("fork", [0, 2, 4, 6, 8, 10], [(0, 2, 100), (0, 4, 101), (2, 6, 102), (6, 8, 103), (4, 10, 104)]))
    for K in (64, 65, 257):
        order = [n for i in reversed(range(K)) for n in (4 * i, 4 * i + 2)]
        cases.append(("pairs_%d_heads_against_ids" % K, order, [(4 * i, 4 * i + 2, 100 + i % 9) for i in range(K)]))
    cases.append(("path_and_its_mirror_interleaved", [0, 7, 2, 5, 4, 3, 6, 1], chain([0, 2, 4, 6]) + chain([7, 5, 3, 1], 200)))
    cases.append(("empty", [], []))
    cases.append(("nodes_without_edges", [4, 2, 0], []))
    cases.append(("overflow", [0, 2, 4, 6, 8, 10], [(0, 2, 2**30), (2, 4, 2**30), (4, 6, 2**30), (6, 8, 5), (6, 10, 6)]))
    return cases


def direct_case(name, order, edges, totals):
    g = MergeGraph(edge_len="weight", overlap_len="overlap_len")
    for n in (order if order is not None else []):
        g._node(P(n))
    for u, v, w in edges:
        g.add_edge(P(u), P(v), {"weight": w, "overlap_len": 17})
    case_order = [int(n) for n in g]
    e_all = mdg.edge_array(g, int).tolist()
    n_ids = max([0] + case_order) + 2
    lengths = [mu.direct_length(n) for n in range(n_ids)]
    rec, _ = run_merge(g, int, n_ids, lengths, "a", totals, case_order)
    print("%-40s nodes %6d  %d paths / %d nodes (%d rounds)" % ("direct_" + name, len(case_order), rec["n_merged"], rec["n_nodes_merged"],
                                                               rec["rounds"]))
    return {"name": "direct_" + name, "direct": True, "results": [rec], "order": case_order, "edges": e_all}


def main():
    totals = dict(mu.new_counts(), max_rounds=0, applications=0)
    cases = []
    chains = {c["name"]: c for c in du.load_golden()["cases"] if not c.get("direct")}
    for c in tu.load_golden()["cases"]:
        if not c.get("direct"):
            cases.append(text_case(dict(c, chain_order_left=chains[c["name"]]["chain"]["order_left"]), totals))
    for c in chains.values():
        if c.get("synth", {}).get("kind") == "union":
            cases.append(text_case(dict(c, chain_order_left=c["chain"]["order_left"]), totals))
    reference_alone = dict(totals)
    for synth in ({"kind": "ring", "n": 3}, {"kind": "ring", "n": 40}, {"kind": "lasso", "n": 12, "tail": 8},
                  {"kind": "lasso", "n": 70, "tail": 6}):
        src = {"name": "_".join(str(v) for v in synth.values()), "params": ru.DEFAULT_PARAMS, "synth": synth}
        src["text_sha256"] = ru.text_digest(mu.case_text(src))
        cases.append(text_case(src, totals, own_order=True))
        # the shape the generator's name promises, under the reference's stage 1 and cleaning
        a, b = cases[-1]["results"]
        n = synth["n"]
        if synth["kind"] == "ring":
            assert (a["n_cycle_nodes"], b["n_cycle_nodes"], a["n_merged"], b["n_merged"]) == (2 * n, 2 * n, 0, 0)
        else:
            t = synth["tail"]
            assert (b["n_merged"], b["n_nodes_merged"], b["n_self_loops"], b["n_cycle_nodes"]) == (4, 2 * (n + t), 2, 0)
    text_totals = dict(totals)
    for name, order, edges in direct_inputs():
        cases.append(direct_case(name, order, edges, totals))
    for k in mu.BRANCHES:
        assert totals[k] > 0, "branch %s never taken" % k
    assert totals["max_rounds"] >= 10
    mu.save_golden({"branch_totals": totals, "text_totals": text_totals, "reference_alone": reference_alone, "cases": cases})
    print("totals", totals)
    print("wrote", mu.GOLDEN_FILE, len(cases), "cases", os.path.getsize(mu.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
