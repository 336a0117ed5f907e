"""The contract of po_layout_superbubbles_all (include/phasm_overlap.h) as plain Python, the direct
cases and the loader of tests/golden/superbubble_all_cases.npz.

``definition_all`` evaluates the definition of a superbubble on the WHOLE graph by brute force: for every pair (s, t) the
set reached from s without passing t, the set that reaches t without passing s, their equality, no cycle inside (a
self-loop and an edge t -> s are cycles), minimality.  ``by_partition`` evaluates the same definition on everything
``partition_graph`` yields -- every non-singleton SCC closed by 'r_' / 're_', then the singletons (superbubble_utils) -- and
unites the results: Sung et al.'s partition theorem says the two are equal, the generator asserts it.  ``scheme_all`` is the
device's scheme by root splitting, run synchronously (phasm_amd.cyclic.HostSuperbubblesAll), in the same shape."""
import os
import random

import numpy as np

import components_utils as cu
import partition_utils as pu
import reduce_utils as ru
import superbubble_utils as su
from phasm_amd import cyclic

GOLDEN_FILE = os.path.join(ru.GOLDEN, "superbubble_all_cases.npz")
DIGEST_ABOVE = pu.DIGEST_ABOVE
BRUTE_FORCE_UP_TO = 300          # nodes of one weakly connected component
ENTRANCE, EXIT, NESTED, SELF_LOOP = su.ENTRANCE, su.EXIT, su.NESTED, su.SELF_LOOP
NONE = su.NONE
ARRAY_KEYS = su.ARRAY_KEYS
STAT_KEYS = ("n_nodes", "n_edges", "n_bubbles", "n_nested", "n_cyclic_bubbles")
SCHEME_KEYS = ("n_split", "n_split_levels", "n_rootless", "n_root_runs", "n_certified", "n_edge_filtered")


def _bits(m):
    while m:
        low = m & -m
        yield low.bit_length() - 1
        m ^= low


def _reach(start, stop, nbr):
    """The nodes reached from ``start`` along ``nbr`` (bit masks) without walking on from ``stop``, both included."""
    seen, frontier = 1 << start, 1 << start
    while frontier:
        nxt = 0
        for v in _bits(frontier):
            if v != stop:
                nxt |= nbr[v]
        frontier = nxt & ~seen
        seen |= frontier
    return seen


def _acyclic(mask, succ):
    """G[mask] has no cycle (a self-loop is one): peel nodes without a predecessor inside."""
    indeg = {v: 0 for v in _bits(mask)}
    for v in indeg:
        if succ[v] >> v & 1:
            return False
        for c in _bits(succ[v] & mask):
            indeg[c] += 1
    todo = [v for v, d in indeg.items() if d == 0]
    for v in todo:
        for c in _bits(succ[v] & mask):
            indeg[c] -= 1
            if indeg[c] == 0:
                todo.append(c)
    return len(todo) == len(indeg)


def brute_force(k, pairs_uv, ends):
    """The superbubbles of a graph on nodes 0..k-1 whose ends lie among ``ends``: {s: (t, U as a bit mask)}."""
    succ, pred = [0] * k, [0] * k
    for a, b in pairs_uv:
        succ[a] |= 1 << b
        pred[b] |= 1 << a
    found = {}
    for s in ends:
        down = _reach(s, -1, succ)
        ok = {}
        for t in ends:
            if t == s or not down >> t & 1:
                continue
            u = _reach(s, t, succ)
            if not u >> t & 1 or u != _reach(t, s, pred):                # (1), (2)
                continue
            if not _acyclic(u, succ):                                     # (3): G[U] holds the edge t -> s, if there is one
                continue
            ok[t] = u
        for t, u in ok.items():                                           # (4)
            if not any(t2 != t and u >> t2 & 1 for t2 in ok):
                assert s not in found, "a node enters two superbubbles"
                found[s] = (t, u)
    assert len({t for t, _ in found.values()}) == len(found), "a node exits two superbubbles"
    return found


def _result(order, eu, ev, found, scc_low):
    """found: {entrance rank: (exit rank, U as a mask of ranks)} -> everything the call returns."""
    n = len(order)
    node_exit, node_inside, flags = np.full(n, NONE, np.int64), np.full(n, NONE, np.int64), np.zeros(n, np.int64)
    for a, b in zip(eu, ev):
        if a == b:
            flags[a] |= SELF_LOOP
    size = {s: bin(u).count("1") - 2 for s, (_, u) in found.items()}
    holder = {}
    for s, (t, u) in found.items():
        for v in _bits(u):
            if v != s and v != t and (v not in holder or size[s] < size[holder[v]]):
                holder[v] = s
    for s, (t, _) in found.items():
        node_exit[s] = order[t]
        flags[s] |= ENTRANCE | (NESTED if s in holder else 0)
        flags[t] |= EXIT
    for v, s in holder.items():
        node_inside[v] = order[s]
    ent = sorted(found)
    count = {}
    for r in scc_low:
        count[r] = count.get(r, 0) + 1
    stats = {"n_nodes": n, "n_edges": len(eu), "n_bubbles": len(ent), "n_nested": sum(1 for s in ent if s in holder),
             "n_cyclic_bubbles": sum(1 for s in ent if count[scc_low[s]] > 1)}
    return {"node_exit": node_exit, "node_inside": node_inside, "node_flags": flags,
            "b_entrance": np.asarray([order[s] for s in ent], np.int64), "b_exit": np.asarray([order[found[s][0]] for s in ent], np.int64),
            "b_inside": np.asarray([size[s] for s in ent], np.int64), "b_nested": np.asarray([int(s in holder) for s in ent], np.int64),
            "stats": stats}


def _graph(edges, order):
    order, eu, ev = pu._ranks(edges, order)
    succ = [[] for _ in order]
    for a, b in zip(eu, ev):
        succ[a].append(b)
    return order, eu, ev, pu.tarjan(len(order), succ)


def _weak(n, eu, ev):
    p = list(range(n))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x
    for a, b in zip(eu, ev):
        a, b = find(a), find(b)
        if a != b:
            p[max(a, b)] = min(a, b)
    groups = {}
    for r in range(n):
        groups.setdefault(find(r), []).append(r)
    return list(groups.values())


def small_enough(edges, order):
    order, eu, ev = pu._ranks(edges, order)
    return all(len(g) <= BRUTE_FORCE_UP_TO for g in _weak(len(order), eu, ev))


def _components(order, eu, ev):
    """Per weakly connected component: its ranks (ascending) and its edges as rank pairs."""
    groups = _weak(len(order), eu, ev)
    where = {}
    for i, ranks in enumerate(groups):
        for r in ranks:
            where[r] = i
    mine = [[] for _ in groups]
    for a, b in zip(eu, ev):
        mine[where[a]].append((a, b))
    return list(zip(groups, mine))


def definition_all(edges, order):
    """edges: rows that start with (u, v); order: the graph's nodes in node order.  The shape of superbubble_utils.definition;
    ``stats``: STAT_KEYS.  Brute force per weakly connected component (a superbubble lies inside one)."""
    order, eu, ev, low = _graph(edges, order)
    found = {}
    for ranks, pairs in _components(order, eu, ev):
        at = {r: i for i, r in enumerate(ranks)}
        for s, (t, u) in brute_force(len(ranks), [(at[a], at[b]) for a, b in pairs], range(len(ranks))).items():
            found[ranks[s]] = (ranks[t], sum(1 << ranks[v] for v in _bits(u)))
    return _result(order, eu, ev, found, low)


def by_partition(edges, order):
    """The same definition on every partition of ``partition_graph``, per weakly connected component as the reference calls
    it: each non-singleton SCC with 'r_' before the nodes that an edge enters from outside and 're_' behind those an edge
    leaves to outside, brute-forced here; the singletons by superbubble_utils.definition.  The union, in the same shape."""
    order, eu, ev, low = _graph(edges, order)
    members = {}
    for r in range(len(order)):
        members.setdefault(low[r], []).append(r)
    found = {}
    for c, ranks in members.items():
        if len(ranks) == 1:
            continue
        at = {r: i for i, r in enumerate(ranks)}
        k = len(ranks)
        R, RE = k, k + 1
        mine = set()
        for a, b in zip(eu, ev):
            if a in at and b in at:
                mine.add((at[a], at[b]))
            elif b in at:
                mine.add((R, at[b]))
            elif a in at:
                mine.add((at[a], RE))
        for s, (t, u) in brute_force(k + 2, sorted(mine), range(k)).items():
            assert not u >> R & 1 and not u >> RE & 1
            found[ranks[s]] = (ranks[t], sum(1 << ranks[v] for v in _bits(u)))
    rank = {x: r for r, x in enumerate(order)}
    for ranks, pairs in _components(order, eu, ev):
        if all(len(members[low[r]]) > 1 for r in ranks):
            continue                      # (no singleton: the acyclic partition is empty)
        sub_order = [order[r] for r in ranks]
        sub_edges = [(order[a], order[b]) for a, b in pairs]
        single = su.definition(sub_edges, sub_order)
        for s, t, nodes in zip(single["b_entrance"].tolist(), single["b_exit"].tolist(), su.node_sets(single, sub_order)):
            found[rank[s]] = (rank[t], sum(1 << rank[x] for x in nodes))
    return _result(order, eu, ev, found, low)


def as_result(host, out):
    """What HostSuperbubblesAll / the device returns in the shape of ``definition_all``."""
    node_exit, node_inside, flags, table = out
    node = lambda a: np.where(np.asarray(a) == 0xFFFFFFFF, NONE, np.asarray(a).astype(np.int64))   # noqa: E731
    return {"node_exit": node(node_exit), "node_inside": node(node_inside), "node_flags": np.asarray(flags).astype(np.int64),
            "b_entrance": table["entrance"].astype(np.int64), "b_exit": table["exit"].astype(np.int64),
            "b_inside": table["n_inside"].astype(np.int64), "b_nested": table["nested"].astype(np.int64), "stats": dict(host)}


def scheme_all(edges, order):
    """The device's scheme run synchronously; ``stats`` gains SCHEME_KEYS, ``roots_of_runs`` what each run split first in
    every rootless SCC."""
    host = cyclic.HostSuperbubblesAll(edges, order)
    res = as_result({}, host.layout_superbubbles_all())
    res["stats"] = host.superbubble_all_stats()
    res["roots_of_runs"] = host.roots_of_runs
    res["situations"] = dict(host.situations)
    return res


def singleton_part(res, edges, order):
    """The entries of a result on the nodes whose SCC is a singleton, in the shape of superbubble_utils.definition: what
    po_layout_superbubbles reports."""
    order, eu, ev, low = _graph(edges, order)
    count = {}
    for r in low:
        count[r] = count.get(r, 0) + 1
    single = np.asarray([count[r] == 1 for r in low], bool)
    rank = {x: r for r, x in enumerate(order)}
    keep = np.asarray([bool(single[rank[s]]) for s in res["b_entrance"].tolist()], bool)
    return {"node_exit": np.where(single, res["node_exit"], NONE), "node_inside": np.where(single, res["node_inside"], NONE),
            "node_flags": np.where(single, res["node_flags"], 0),
            "b_entrance": res["b_entrance"][keep], "b_exit": res["b_exit"][keep], "b_inside": res["b_inside"][keep],
            "b_nested": res["b_nested"][keep]}


def check_singleton_part(res, old, edges, order):
    """``old``: a superbubble_utils.definition-shaped result of po_layout_superbubbles on the same graph.  A superbubble lies
    inside one partition, so on singleton nodes both calls say the same; on the others the old call says nothing."""
    part = singleton_part(res, edges, order)
    for k in ARRAY_KEYS:
        assert np.asarray(part[k]).tolist() == np.asarray(old[k]).tolist(), "singleton part: " + k
    order, eu, ev, low = _graph(edges, order)
    count = {}
    for r in low:
        count[r] = count.get(r, 0) + 1
    for r in range(len(order)):
        if count[low[r]] > 1:      # (the old call flags self-loops on singletons only)
            assert old["node_exit"][r] == NONE and old["node_inside"][r] == NONE and old["node_flags"][r] == 0


# ---- direct cases: edges (u, v) plus an explicit node order ---------------------------------------------------------------

def _diamond(s, a, b, t):
    return [(s, a), (s, b), (a, t), (b, t)]


SEVEN = [(1, 0), (0, 3), (1, 2), (2, 3), (3, 4), (4, 1), (3, 5), (5, 1), (4, 6), (6, 4)]   # a=0 s=1 b=2 t=3 p=4 q=5 p'=6


def four_node_union():
    """All 4 096 loop-free digraphs on 4 labelled nodes as one graph: copy k has the nodes 8k, 8k + 2, 8k + 4, 8k + 6 and the
    edges whose bit is set in k."""
    slots = [(a, b) for a in range(4) for b in range(4) if a != b]
    order, edges = [], []
    for k in range(4096):
        order += [8 * k + 2 * i for i in range(4)]
        edges += [(8 * k + 2 * a, 8 * k + 2 * b) for i, (a, b) in enumerate(slots) if k >> i & 1]
    return order, edges


def strong_union(count=2000, seed=7):
    """``count`` random strongly connected digraphs of 5 to 10 nodes, disjoint: a Hamiltonian cycle in a random order plus
    a few random chords."""
    rng = random.Random(seed)
    order, edges, at = [], [], 0
    for _ in range(count):
        k = rng.randrange(5, 11)
        ids = [2 * (at + i) for i in range(k)]
        at += k
        ring = list(ids)
        rng.shuffle(ring)
        es = set(pu._ring(ring))
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            a, b = rng.sample(ids, 2)
            es.add((a, b))
        shuffled = list(ids)
        rng.shuffle(shuffled)
        order += shuffled
        edges += sorted(es, key=lambda e: rng.random())
    return order, edges


def ring_of_diamonds(k, at=0):
    """k diamonds in a ring: the exit of one is the entrance of the next.  Diamond i: 6i -> 6i + 2 / 6i + 4 -> 6i + 6."""
    edges = []
    for i in range(k):
        s, t = at + 6 * i, at + 6 * ((i + 1) % k)
        edges += _diamond(s, s + 2, s + 4, t)
    return [at + 2 * i for i in range(3 * k)], edges


def direct_inputs():
    """(name, order, edges, n_ids or None): the shapes this call is about, then the direct cases of superbubble_utils (which
    begin with those of partition_utils).  Nodes are even ids."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    new = [("two_cycle", [0, 2], [(0, 2), (2, 0)]), ("three_ring", [0, 2, 4], pu._ring([0, 2, 4]))]
    # a ring with one diamond: 0 -> 2 | 4 -> 6 -> 8 -> 0; the lowest rank is the entrance, the exit, an interior node, outside
    one = _diamond(0, 2, 4, 6) + [(6, 8), (8, 0)]
    for tag, first in (("entrance", 0), ("exit", 6), ("interior", 2), ("outside", 8)):
        new.append(("ring_with_a_diamond_lowest_is_the_" + tag, [first] + [x for x in ev(5) if x != first], one))
    for low in range(7):
        new.append(("seven_nodes_lowest_%d" % low, [2 * low] + [2 * x for x in range(7) if x != low], [(2 * a, 2 * b) for a, b in SEVEN]))
    # a bubble nested in a bubble on a ring: 0 -> 2 -> (4 | 6) -> 8 -> 12, 0 -> 10 -> 12, 12 -> 14 -> 0; the innermost interior first
    nested = [(0, 2), (0, 10), (10, 12), (8, 12), (12, 14), (14, 0)] + _diamond(2, 4, 6, 8)
    new.append(("nested_on_a_ring_innermost_interior_lowest", [4] + [x for x in ev(8) if x != 4], nested))
    new.append(("nested_on_a_ring_ascending", ev(8), nested))
    # a diamond plus the edge t -> s inside a larger SCC
    new.append(("diamond_with_the_edge_back_in_an_scc", ev(6), _diamond(2, 4, 6, 8) + [(8, 2), (8, 10), (10, 0), (0, 2)]))
    for tag, x in (("entrance", 0), ("exit", 6), ("interior", 4)):
        new.append(("ring_self_loop_on_the_" + tag, [8, 0, 2, 4, 6], one + [(x, x)]))
    # an SCC with several R_IN nodes, a bubble behind each: two tails enter the ring 0 .. 14 at 0 and at 8
    ring = _diamond(0, 2, 4, 6) + [(6, 8)] + _diamond(8, 10, 12, 14) + [(14, 0)]
    new.append(("several_r_in", [20, 22] + ev(8), ring + [(20, 0), (22, 8)]))
    new.append(("only_re_out", ev(8) + [20], ring + [(6, 20)]))
    new.append(("r_in_and_re_out", [20] + ev(8) + [22], ring + [(20, 8), (6, 22)]))
    # cycle -> bridge -> cycle, with bubbles in all three
    o1, e1 = ring_of_diamonds(2)
    o2, e2 = ring_of_diamonds(2, 100)
    bridge = _diamond(40, 42, 44, 46)
    new.append(("cycle_bridge_cycle_with_bubbles", o1 + ev(4, 40) + o2, e1 + [(6, 40)] + bridge + [(46, 100)] + e2))
    for k in (3, 16):
        o, e = ring_of_diamonds(k)
        new.append(("ring_of_%d_diamonds" % k, o, e))
        new.append(("ring_of_%d_diamonds_interior_lowest" % k, [o[1]] + [o[0]] + o[2:], e))
    o, e = ring_of_diamonds(40)
    new.append(("ring_of_40_diamonds_scrambled", pu._scrambled(o, 40), e))
    o, e = four_node_union()
    new.append(("four_node_digraphs_4096", o, e))
    o, e = strong_union()
    new.append(("strong_union_2000", o, e))
    return [("cy_" + name, order, edges, None) for name, order, edges in new] + list(su.direct_inputs())


# ---- golden file ---------------------------------------------------------------------------------------------------

def record_of(res):
    """The golden record of one application: the stats and the arrays, or above DIGEST_ABOVE edges their digest."""
    rec = {k: int(res["stats"][k]) for k in STAT_KEYS + SCHEME_KEYS}
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = cu.digest(*[res[k] for k in ARRAY_KEYS])
    else:
        for k in ARRAY_KEYS:
            rec["a_" + k] = np.asarray(res[k]).tolist()
    return rec


def check_against_record(res, rec, keys=STAT_KEYS + SCHEME_KEYS):
    """A ``definition_all``-shaped result (of any producer) against one golden record."""
    assert {k: int(res["stats"][k]) for k in keys} == {k: rec[k] for k in keys}
    if "sha256" in rec:
        assert cu.digest(*[np.asarray(res[k], np.int64) for k in ARRAY_KEYS]) == rec["sha256"]
    else:
        for k in ARRAY_KEYS:
            assert np.asarray(res[k], np.int64).tolist() == list(rec["a_" + k]), k


def scrambled_edges(edges, seed=11):
    out = list(edges)
    random.Random(seed).shuffle(out)
    return out


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]

