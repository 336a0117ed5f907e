"""The contract of po_layout_bubblechains (include/phasm_overlap.h) as plain Python, the scheme the
kernels use run synchronously, the direct cases and the loader of tests/golden/bubblechain_cases.npz.

``definition`` restates the reference's sequential walk (build_bubblechains, phasm/assembly_graph.py:594-652) on the arrays of
``superbubble_utils.scheme``: the bubbles without NESTED, the three-tier start list, the walk from exit to entrance with its
``visited`` set, ``superbubble_nodes`` as the chains of ``node_inside``, ``networkx.subgraph`` as the edges with both ends
in the node set.  ``scheme`` reaches the same the way the device does (phasm_amd/csrc/bubblechains.hip.h): top-level
entrances, their links, pointer jumping to the outermost holder, list ranking toward the heads, sums at the heads."""
import os

import numpy as np

import components_utils as cu
import partition_utils as pu
import reduce_utils as ru
import superbubble_utils as su

GOLDEN_FILE = os.path.join(ru.GOLDEN, "bubblechain_cases.npz")
DIGEST_ABOVE = su.DIGEST_ABOVE
NONE = su.NONE
ARRAY_KEYS = ("node_chain", "node_bubble", "edge_chain", "c_first", "c_last", "c_bubbles", "c_nodes", "c_edges")
STAT_KEYS = ("n_nodes", "n_edges", "n_bubbles", "n_top", "n_chains", "n_short", "n_chain_nodes", "n_chain_edges", "max_chain_bubbles")
SCHEME_KEYS = ("n_nest_rounds", "n_chain_rounds", "n_levels_forward")


def _result(order, eu, ev, sb, chains, min_nodes):
    """Everything the call returns.  chains: (head rank, last exit rank, bubbles, {rank: position}) of EVERY chain."""
    n = len(order)
    chains = sorted(chains, key=lambda c: c[0])                         # numbered by the rank of their heads
    kept = [c for c in chains if len(c[3]) >= min_nodes]
    node_chain, node_bubble = np.full(n, NONE, np.int64), np.full(n, NONE, np.int64)
    for j, (_, _, _, pos) in enumerate(kept):
        for r, k in pos.items():
            assert node_chain[r] == NONE, "a node lies in two chains"
            node_chain[r], node_bubble[r] = j, k
    same = (node_chain[eu] == node_chain[ev]) if len(eu) else np.zeros(0, bool)
    edge_chain = np.where(same, node_chain[eu], NONE) if len(eu) else np.zeros(0, np.int64)
    c_edges = np.bincount(edge_chain[edge_chain != NONE], minlength=len(kept)).astype(np.int64)
    stats = {"n_nodes": n, "n_edges": len(eu), "n_bubbles": sb["stats"]["n_bubbles"],
             "n_top": sb["stats"]["n_bubbles"] - sb["stats"]["n_nested"], "n_chains": len(kept), "n_short": len(chains) - len(kept),
             "n_chain_nodes": int((node_chain != NONE).sum()), "n_chain_edges": int(c_edges.sum()),
             "max_chain_bubbles": max([c[2] for c in chains] + [0])}
    return {"node_chain": node_chain, "node_bubble": node_bubble, "edge_chain": edge_chain,
            "c_first": np.asarray([order[c[0]] for c in kept], np.int64), "c_last": np.asarray([order[c[1]] for c in kept], np.int64),
            "c_bubbles": np.asarray([c[2] for c in kept], np.int64), "c_nodes": np.asarray([len(c[3]) for c in kept], np.int64),
            "c_edges": c_edges, "stats": stats}


def _inputs(edges, order, sb):
    order, eu, ev = pu._ranks(edges, order)
    order = [int(x) for x in order]
    if sb is None:
        sb = su.scheme(edges, order)
    return order, np.asarray(eu, np.int64), np.asarray(ev, np.int64), sb, {x: r for r, x in enumerate(order)}


# ---- the reference's walk -------------------------------------------------------------------------------------------------

def definition(edges, order, min_nodes=1, sb=None):
    """edges: rows that start with (u, v); order: the graph's nodes in node order; sb: ``superbubble_utils.scheme`` of them.
    Returns ``node_chain`` / ``node_bubble`` parallel to ``order`` and ``edge_chain`` parallel to ``edges`` (NONE where there
    is none), the chain table ``c_first`` / ``c_last`` / ``c_bubbles`` / ``c_nodes`` / ``c_edges`` in chain order, ``stats``."""
    order, eu, ev, sb, rank = _inputs(edges, order, sb)
    n = len(order)
    top = [i for i, nested in enumerate(sb["b_nested"].tolist()) if not nested]      # find_superbubbles(g, report_nested=False)
    bubbles = {rank[int(sb["b_entrance"][i])]: rank[int(sb["b_exit"][i])] for i in top}
    sets = su.node_sets(sb, order)
    nodes_of = {rank[int(sb["b_entrance"][i])]: [rank[x] for x in sets[i]] for i in top}   # superbubble_nodes(g, s, t)
    entrances, exits = sorted(bubbles), set(bubbles.values())
    in_degree = np.bincount(ev, minlength=n) if n else np.zeros(0, np.int64)
    tiers = [[s for s in entrances if in_degree[s] == 0], [s for s in entrances if s not in exits], list(entrances)]
    visited, chains = set(), []
    for tier, starts in enumerate(tiers):
        for start in starts:
            head, pos, num_bubbles, last = start, {}, 0, NONE
            while start in bubbles:
                bubble_exit = bubbles[start]
                if start in visited and bubble_exit in visited:
                    break
                for x in nodes_of[start]:
                    if x not in pos or x == start:       # (an exit that enters the next bubble lies at that one's position)
                        pos[x] = num_bubbles
                visited.update(nodes_of[start])
                start, last = bubble_exit, bubble_exit
                num_bubbles += 1
            if num_bubbles:
                assert tier < 2, "a start of the third tier builds a chain"
                chains.append((head, last, num_bubbles, pos))
    return _result(order, eu, ev, sb, chains, min_nodes)


# ---- the device's scheme, run synchronously -------------------------------------------------------------------------------

def scheme(edges, order, min_nodes=1, sb=None):
    """The same by the device's scheme; ``stats`` gains the round counts of the two pointer-jumping loops (closing rounds
    included; 0 for a loop the device does not run) and the forward levels of the superbubble stage."""
    order, eu, ev, sb, rank = _inputs(edges, order, sb)
    n = len(order)
    to_rank = lambda a: np.asarray([rank[int(x)] if x != NONE else NONE for x in a], np.int64)   # noqa: E731
    exit_of, inside = to_rank(sb["node_exit"]), to_rank(sb["node_inside"])
    enters = (sb["node_flags"] & su.ENTRANCE) != 0
    top_ent = enters & (inside == NONE)
    nxt, pred = np.full(n, NONE, np.int64), np.full(n, NONE, np.int64)
    for s in np.flatnonzero(top_ent).tolist():
        t = int(exit_of[s])
        assert pred[t] == NONE, "a node exits two top-level bubbles"
        pred[t] = s
        if top_ent[t]:
            nxt[s] = t
    linked = top_ent & (pred != NONE)
    head, last_exit = top_ent & ~linked, ~top_ent & (pred != NONE)
    # the outermost holder: top[v] = top[top[v]] while that exists
    top, nest_rounds = inside.copy(), 0
    if top_ent.any() and sb["stats"]["n_nested"]:
        while True:
            assert nest_rounds < sb["stats"]["n_nested"] + 2, "the holder rounds reached their cap"
            nest_rounds += 1
            held = np.flatnonzero(top != NONE)
            up = top[top[held]]
            move = up != NONE
            if not move.any():
                break
            new = top.copy()
            new[held[move]] = up[move]
            top = new
    # list ranking toward the heads: hops += hops[jb]; jb = jb[jb]
    ranks = np.arange(n, dtype=np.int64)
    jb, hops, chain_rounds = np.where(linked, pred, ranks), linked.astype(np.int64), 0
    if top_ent.any():
        while True:
            assert chain_rounds < int(top_ent.sum()) + 2, "the ranking rounds reached their cap"
            chain_rounds += 1
            jj = jb[jb]
            moved = bool((jj != jb).any())
            jb, hops = jj, hops + hops[jb]
            if not moved:
                break
    chains = {h: [h, NONE, 0, {}] for h in np.flatnonzero(head).tolist()}
    for r in range(n):
        s = r if top_ent[r] else int(pred[r]) if last_exit[r] else int(top[r])
        if s == NONE:
            continue
        assert top_ent[s] and head[jb[s]], "a holder reached no head"
        c = chains[int(jb[s])]
        c[3][r] = int(hops[s])
        if top_ent[r]:
            c[2] += 1
            if nxt[r] == NONE:
                c[1] = int(exit_of[r])
    res = _result(order, eu, ev, sb, [tuple(c) for c in chains.values()], min_nodes)
    res["stats"].update({"n_nest_rounds": nest_rounds, "n_chain_rounds": chain_rounds,
                         "n_levels_forward": sb["stats"]["n_levels_forward"]})
    return res


def log2_ceil(x):
    return max(int(x) - 1, 0).bit_length()


def round_bounds(stats):
    """What the issue bounds the two loops by: (nest rounds, chain rounds)."""
    return log2_ceil(max(stats["n_levels_forward"], 2)) + 2, log2_ceil(max(stats["max_chain_bubbles"], 2)) + 2


def nodes_of(res, order, j):
    """The nodes of chain ``j`` in node order."""
    return [int(x) for x, c in zip(order, res["node_chain"].tolist()) if c == j]


def bubbles_of(res, order, sb, j):
    """The (entrance, exit) pairs of chain ``j`` in chain order."""
    exit_of = dict(zip([int(x) for x in order], sb["node_exit"].tolist()))
    out, s = [], int(res["c_first"][j])
    for _ in range(int(res["c_bubbles"][j])):
        out.append((s, int(exit_of[s])))
        s = int(exit_of[s])
    return out


# ---- direct cases: edges (u, v), an explicit node order, min_nodes ----------------------------------------------------------

def direct_inputs():
    """(name, order, edges, n_ids or None, min_nodes): the direct cases of superbubble_utils with min_nodes 1 (they hold the
    paths of 1 025 nodes in three orders, the two diamonds sharing a node, nesting depth 3, the nested-with-outer-discarded
    case, the fan-out-and-in of 257, the 2 050 disjoint edges, the 3-cycle with tails and the empty graph), then the shapes
    this stage is about.  Nodes are even ids."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    D = su._diamond
    cases = [(name, order, edges, n_ids, 1) for name, order, edges, n_ids in su.direct_inputs()]
    new = []
    # two chains in one component, joined by the fork at 40, which enters no bubble (its branches never meet): the head that
    # ranks first has the higher id
    new.append(("two_chains_heads_descending", [20, 22, 24, 40, 0, 2, 4], [(40, 20), (40, 0), (20, 22), (22, 24), (0, 2), (2, 4)], 1))
    # a head with in-degree 0 (node 0), and a head with two in-edges (node 10: from the first chain's last exit and from 6)
    new.append(("head_with_and_without_in_edges", [0, 2, 4, 6, 10, 12, 14], [(0, 2), (2, 4), (4, 10), (6, 10), (10, 12), (12, 14)], 1))
    # diamond, edge, diamond; then a fork that is no bubble
    new.append(("diamond_edge_diamond_fork", pu._scrambled(ev(10), 7), D(0, 2, 4, 6) + [(6, 8)] + D(8, 10, 12, 14) + [(14, 16), (14, 18)], 1))
    # nesting depth 3 inside a chain member: a diamond, then the three bubbles inside one another, then an edge
    depth3 = [(2, 4), (4, 26), (2, 6), (6, 8), (8, 10), (10, 22), (8, 12)] + D(12, 14, 16, 18) + [(18, 20), (20, 22), (22, 24), (24, 26)]
    new.append(("nesting_depth_3_inside_a_chain_member", pu._scrambled(ev(14, 2) + [40, 42, 44, 46], 3),
                D(40, 42, 44, 2) + depth3 + [(26, 46)], 1))
    # nesting depth 300: bubble k enters at 4k and exits at 4k + 2 ... mirrored: s_k -> s_(k+1), s_k -> t_k, t_(k+1) -> t_k
    n = 300
    s_of, t_of = (lambda k: 4 * k), (lambda k: 4 * k + 2)
    deep = []
    for k in range(n - 1):
        deep += [(s_of(k), s_of(k + 1)), (t_of(k + 1), t_of(k)), (s_of(k), t_of(k))]
    deep += [(s_of(n - 1), t_of(n - 1))]
    new.append(("nesting_depth_300", pu._scrambled([s_of(k) for k in range(n)] + [t_of(k) for k in range(n)], 300), deep, 1))
    for m in (257,):       # (1 025 in three orders is among the reused cases)
        ids = ev(m)
        for tag, order in (("ascending", ids), ("descending", ids[::-1]), ("scrambled", pu._scrambled(ids, m))):
            new.append(("path_%d_%s" % (m, tag), order, pu._path(ids), 1))
    new.append(("self_loop_on_a_middle_node_of_a_path", ev(9), pu._path(ev(9)) + [(8, 8)], 1))
    small = [(4 * i, 4 * i + 2) for i in range(5)] + D(100, 102, 104, 106)
    new.append(("min_nodes_3_on_disjoint_edges_plus_a_diamond", ev(10) + [100, 102, 104, 106], small, 3))
    new.append(("min_nodes_above_every_chain", ev(10) + [100, 102, 104, 106], small, 5))
    new.append(("min_nodes_above_every_chain_of_a_long_path", pu._scrambled(ev(40), 2), pu._path(ev(40)), 41))
    return cases + [("bc_" + name, order, edges, None, min_nodes) for name, order, edges, min_nodes in new]


# ---- golden file ---------------------------------------------------------------------------------------------------

def _canonical(res, edges):
    """The arrays of a result with ``edge_chain`` in the order of the edges sorted by (u, v): what a record holds, whatever
    order the producer's graph keeps its edges in (a graph has no edge twice)."""
    e = cu.uv_of(edges)
    by = np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, np.int64)
    return [np.asarray(res[k], np.int64)[by] if k == "edge_chain" else np.asarray(res[k], np.int64) for k in ARRAY_KEYS]


def record_of(res, edges):
    """The golden record of one application: the stats and the arrays, or above DIGEST_ABOVE edges their digest."""
    rec = {k: res["stats"][k] for k in STAT_KEYS}
    arrays = _canonical(res, edges)
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = cu.digest(*arrays)
    else:
        for k, a in zip(ARRAY_KEYS, arrays):
            rec["a_" + k] = a.tolist()
    return rec


def check_against_record(res, rec, edges):
    """A ``definition``-shaped result (of any producer, on ``edges`` in its own order) against one golden record."""
    assert {k: int(res["stats"][k]) for k in STAT_KEYS} == {k: rec[k] for k in STAT_KEYS}
    arrays = _canonical(res, edges)
    if "sha256" in rec:
        assert cu.digest(*arrays) == rec["sha256"]
    else:
        for k, a in zip(ARRAY_KEYS, arrays):
            assert a.tolist() == list(rec["a_" + k]), k


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]
