"""The contract of po_layout_superbubbles (include/phasm_overlap.h) as plain Python, the scheme the
kernels use run synchronously, the direct cases and the loader of tests/golden/superbubble_cases.npz.

``definition`` evaluates the definition of a superbubble (Onodera et al.: reachability, matching, acyclicity, minimality)
by brute force on the partition graph P, 'r_' and 're_' included.  ``scheme`` reaches the same pairs the way the device does
(phasm_amd/csrc/superbubbles.hip.h): longest-path levels, the dominator and the post-dominator tree level by level, the
pairs (s, t) with t == ipdom[s] and s == idom[t], the innermost enclosing bubble, the discards for self-loops."""
import os
import random

import numpy as np

import components_utils as cu
import partition_utils as pu
import reduce_utils as ru

GOLDEN_FILE = os.path.join(ru.GOLDEN, "superbubble_cases.npz")
DIGEST_ABOVE = pu.DIGEST_ABOVE
BRUTE_FORCE_UP_TO = 300          # nodes of the graph
ENTRANCE, EXIT, NESTED, SELF_LOOP = 1, 2, 4, 8
NONE = -1
ARRAY_KEYS = ("node_exit", "node_inside", "node_flags", "b_entrance", "b_exit", "b_inside", "b_nested")
STAT_KEYS = ("n_nodes", "n_edges", "n_p_nodes", "n_p_edges", "n_bubbles", "n_nested", "n_self_loop_nodes", "n_discarded")
SCHEME_KEYS = ("n_levels_forward", "n_levels_backward", "n_level_rounds", "n_discard_rounds", "n_survivors_in_discarded")


def _structure(edges, order):
    """The partition graph by rank: real (singleton) ranks, the edges of D, the self-loops, and who hangs on 'r_' / 're_'."""
    part = pu.partition(edges, order)
    order, eu, ev = pu._ranks(edges, order)
    n = len(order)
    single = (part["n_nodes"] == 1)[part["node_scc"]] if n else np.zeros(0, bool)
    flags = part["node_flags"]
    loop, parents, children = [False] * n, [[] for _ in range(n)], [[] for _ in range(n)]
    n_class1 = 0
    for e, (a, b) in enumerate(zip(eu, ev)):
        if part["edge_class"][e] != 1:
            continue
        n_class1 += 1
        if a == b:
            loop[a] = True
        else:
            parents[b].append(a)
            children[a].append(b)
    real = [bool(x) for x in single]
    r_in = [real[r] and bool(flags[r] & (pu.R_IN | pu.START)) for r in range(n)]
    re_out = [real[r] and bool(flags[r] & (pu.RE_OUT | pu.SINK)) for r in range(n)]
    stats = {"n_nodes": n, "n_edges": len(eu), "n_p_nodes": sum(real) + any(r_in) + any(re_out),
             "n_p_edges": n_class1 + sum(r_in) + sum(re_out), "n_self_loop_nodes": sum(loop)}
    return order, flags, real, loop, parents, children, r_in, re_out, stats


def _result(order, loop, stats, pairs, inside_of, nested, n_inside, n_discarded):
    """Everything the call returns.  pairs: {entrance rank: exit rank}; inside_of: {rank: entrance rank of the innermost
    bubble that holds it strictly}; nested: set of entrance ranks; n_inside: {entrance rank: count}."""
    n = len(order)
    node_exit, node_inside, flags = np.full(n, NONE, np.int64), np.full(n, NONE, np.int64), np.zeros(n, np.int64)
    for r in range(n):
        if loop[r]:
            flags[r] |= SELF_LOOP
    for s, t in pairs.items():
        node_exit[s] = order[t]
        flags[s] |= ENTRANCE | (NESTED if s in nested else 0)
        flags[t] |= EXIT
    for v, s in inside_of.items():
        node_inside[v] = order[s]
    ent = sorted(pairs)
    st = dict(stats)
    st.update({"n_bubbles": len(ent), "n_nested": len(nested), "n_discarded": n_discarded})
    return {"node_exit": node_exit, "node_inside": node_inside, "node_flags": flags,
            "b_entrance": np.asarray([order[s] for s in ent], np.int64), "b_exit": np.asarray([order[pairs[s]] for s in ent], np.int64),
            "b_inside": np.asarray([n_inside[s] for s in ent], np.int64), "b_nested": np.asarray([int(s in nested) for s in ent], np.int64),
            "stats": st}


# ---- the definition, by brute force ---------------------------------------------------------------------------------------

def definition(edges, order):
    """edges: rows that start with (u, v); order: the graph's nodes in node order.  Returns ``node_exit`` / ``node_inside``
    (node ids, NONE where there is none) and ``node_flags`` parallel to ``order``, the bubble table ``b_entrance`` /
    ``b_exit`` / ``b_inside`` / ``b_nested`` in the order of the entrances' ranks, and ``stats``."""
    order, _, real, loop, parents, children, r_in, re_out, stats = _structure(edges, order)
    n = len(order)
    ranks = [r for r in range(n) if real[r]]
    k = len(ranks)
    at = {r: i for i, r in enumerate(ranks)}
    R, RE = k, k + 1
    ch, pa = [[] for _ in range(k + 2)], [[] for _ in range(k + 2)]
    for r in ranks:
        for c in children[r]:
            ch[at[r]].append(at[c])
            pa[at[c]].append(at[r])
        if r_in[r]:
            ch[R].append(at[r])
            pa[at[r]].append(R)
        if re_out[r]:
            ch[at[r]].append(RE)
            pa[RE].append(at[r])
    loopmask = sum(1 << at[r] for r in ranks if loop[r])
    indeg = [len(p) for p in pa]
    topo = [x for x in range(k + 2) if indeg[x] == 0]
    for x in topo:
        for c in ch[x]:
            indeg[c] -= 1
            if indeg[c] == 0:
                topo.append(c)
    assert len(topo) == k + 2, "the partition graph without its self-loops is acyclic"
    fwd, bwd = [None] * k, [None] * k      # fwd[t][x]: reached from x without passing t; bwd[s][x]: reach x without passing s
    for t in range(k):
        f = [0] * (k + 2)
        for x in reversed(topo):
            m = 1 << x
            if x != t:
                for c in ch[x]:
                    m |= f[c]
            f[x] = m
        fwd[t] = f
    for s in range(k):
        b = [0] * (k + 2)
        for x in topo:
            m = 1 << x
            if x != s:
                for p in pa[x]:
                    m |= b[p]
            b[x] = m
        bwd[s] = b

    def minimal(with_loops):
        found = {}
        for s in range(k):
            ok = [t for t in range(k) if t != s and fwd[t][s] >> t & 1 and fwd[t][s] == bwd[s][t]
                  and not (with_loops and fwd[t][s] & loopmask)]
            for t in ok:
                if not any(t2 != t and fwd[t][s] >> t2 & 1 for t2 in ok):
                    assert s not in found, "a node enters two superbubbles"
                    found[s] = t
        return found

    pairs = minimal(True)
    assert len(set(pairs.values())) == len(pairs), "a node exits two superbubbles"
    n_discarded = len(minimal(False)) - len(pairs)
    U = {s: fwd[t][s] for s, t in pairs.items()}
    nested = {s for s, t in pairs.items() if any(s2 != s and U[s2] >> s & 1 and U[s2] >> t & 1 for s2 in pairs)}
    inside_of = {}
    for v in range(k):
        holders = [s for s, t in pairs.items() if v != s and v != t and U[s] >> v & 1]
        if holders:
            inside_of[ranks[v]] = ranks[min(holders, key=lambda s: bin(U[s]).count("1"))]
    n_inside = {ranks[s]: bin(U[s]).count("1") - 2 for s in pairs}
    return _result(order, loop, stats, {ranks[s]: ranks[t] for s, t in pairs.items()}, inside_of, {ranks[s] for s in nested}, n_inside,
                   n_discarded)


# ---- the device's scheme, run synchronously -------------------------------------------------------------------------------

def _levels(n, real, eu, ev):
    """Longest-path levels (1 on every real rank with no edge into it) by edge-parallel max rounds; the closing round counts."""
    lvl = np.where(np.asarray(real, bool), 1, 0).astype(np.int64) if n else np.zeros(0, np.int64)
    rounds, cap = 0, int(sum(real)) + 2
    while True:
        assert rounds < cap, "the level rounds reached their cap"
        rounds += 1
        before = lvl.copy()
        if len(eu):
            np.maximum.at(lvl, ev, before[eu] + 1)
        if np.array_equal(lvl, before):
            return lvl, rounds


def _tree(n, lvl, towards_root, is_top):
    """The dominator tree of the graph whose edges point away from the virtual root ``n``: idom per rank, level by level.
    towards_root[v]: the neighbours of v on the root's side; is_top[v]: v hangs on the root itself."""
    ROOT = n
    idom, depth = [NONE] * (n + 1), [0] * (n + 1)
    idom[ROOT] = ROOT
    by_level = {}
    for r in range(n):
        if lvl[r]:
            by_level.setdefault(int(lvl[r]), []).append(r)

    def lca(a, b, cap):
        steps = 0
        while a != b:
            assert steps <= cap, "the walk along the tree reached its cap"
            steps += 1
            if depth[a] >= depth[b]:
                a = idom[a]
            else:
                b = idom[b]
        return a

    for level in sorted(by_level):
        for v in by_level[level]:
            d = ROOT if is_top[v] else NONE
            for p in towards_root[v]:
                d = p if d == NONE else lca(d, p, 2 * level + 2)
            assert d != NONE
            idom[v] = d
            depth[v] = depth[d] + 1
    return idom, by_level


def scheme(edges, order):
    """The same by the device's scheme; ``stats`` gains the levels, the round counts (closing rounds included; the device
    runs the forward and the backward level rounds in one loop, so it needs about half of ``n_level_rounds``) and the number of
    surviving bubbles whose entrance lies inside a discarded one."""
    order, flags, real, loop, parents, children, _, _, stats = _structure(edges, order)
    n = len(order)
    source = [real[r] and (bool(flags[r] & pu.R_IN) or not parents[r]) for r in range(n)]
    sink = [real[r] and (bool(flags[r] & pu.RE_OUT) or not children[r]) for r in range(n)]
    eu = np.asarray([p for v in range(n) for p in parents[v]], np.int64)
    ev = np.asarray([v for v in range(n) for _ in parents[v]], np.int64)
    lvl_f, rounds_f = _levels(n, real, eu, ev)
    lvl_b, rounds_b = _levels(n, real, ev, eu)
    idom, by_level = _tree(n, lvl_f, parents, source)
    ipdom, _ = _tree(n, lvl_b, children, sink)
    ROOT = n
    exit_of = {s: ipdom[s] for s in range(n) if real[s] and ipdom[s] != ROOT and idom[ipdom[s]] == s}
    encl = [NONE] * (n + 1)
    for level in sorted(by_level):
        for v in by_level[level]:
            d = idom[v]
            if d == ROOT:
                continue
            encl[v] = d if d in exit_of and exit_of[d] != v else encl[d]
    dead = set()
    for v in range(n):
        if loop[v]:
            if v in exit_of:
                dead.add(v)
            if idom[v] != ROOT and exit_of.get(idom[v]) == v:
                dead.add(idom[v])
            if encl[v] != NONE:
                dead.add(encl[v])
    discard_rounds = 0
    while True:
        assert discard_rounds < len(exit_of) + 2, "the discard rounds reached their cap"
        discard_rounds += 1
        more = {encl[s] for s in dead if encl[s] != NONE} - dead
        if not more:
            break
        dead |= more
    pairs = {s: t for s, t in exit_of.items() if s not in dead}
    inside_of = {v: encl[v] for v in range(n) if real[v] and encl[v] != NONE and encl[v] not in dead}
    nested = {s for s in pairs if s in inside_of}
    total = {s: 0 for s in pairs}
    for v, s in inside_of.items():
        total[s] += 1
    for level in sorted(by_level, reverse=True):
        for s in by_level[level]:
            if s in nested:
                total[inside_of[s]] += total[s]
    res = _result(order, loop, stats, pairs, inside_of, nested, total, len(exit_of) - len(pairs))
    res["stats"].update({"n_levels_forward": int(lvl_f.max()) if n else 0, "n_levels_backward": int(lvl_b.max()) if n else 0,
                         "n_level_rounds": rounds_f + rounds_b, "n_discard_rounds": discard_rounds,
                         "n_survivors_in_discarded": sum(1 for s in pairs if encl[s] != NONE and encl[s] in dead)})
    return res


def nodes_of(res, order, entrance):
    """``superbubble_nodes(g, s, t)``: the two ends plus the nodes whose chain of ``node_inside`` reaches the entrance."""
    order = [int(x) for x in order]
    rank = {x: i for i, x in enumerate(order)}
    inside = res["node_inside"]
    out = {int(entrance), int(res["node_exit"][rank[int(entrance)]])}
    for r, x in enumerate(order):
        at, steps = int(inside[r]), 0
        while at != NONE and at != entrance and steps <= len(order):
            at, steps = int(inside[rank[at]]), steps + 1
        if at == entrance:
            out.add(x)
    return out


def node_sets(res, order):
    """The node set of every bubble in table order, in one pass (children of the ``node_inside`` forest)."""
    order = [int(x) for x in order]
    rank = {x: i for i, x in enumerate(order)}
    kids = {}
    for r, s in enumerate(res["node_inside"].tolist()):
        if s != NONE:
            kids.setdefault(s, []).append(order[r])
    out = []
    for s, t in zip(res["b_entrance"].tolist(), res["b_exit"].tolist()):
        members, work = {s, t}, [s]
        while work:
            for x in kids.get(work.pop(), ()):
                members.add(x)
                if res["node_flags"][rank[x]] & ENTRANCE:
                    work.append(x)
        out.append(sorted(members))
    return out


# ---- direct cases: edges (u, v) plus an explicit node order ---------------------------------------------------------------

def _diamond(s, a, b, t):
    return [(s, a), (s, b), (a, t), (b, t)]


def direct_inputs():
    """(name, order, edges, n_ids or None): the direct cases of partition_utils, then the shapes this stage is about.  Nodes
    are even ids."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    cases = list(pu.direct_inputs())
    new = [("single_edge", [0, 2], [(0, 2)]), ("path_3", [0, 2, 4], [(0, 2), (2, 4)])]
    for n in (9, 17, 1025):
        ids = ev(n)
        for tag, order in (("ascending", ids), ("descending", ids[::-1]), ("scrambled", pu._scrambled(ids, n))):
            new.append(("path_%d_%s" % (n, tag), order, pu._path(ids)))
    new.append(("diamond", [0, 2, 4, 6], _diamond(0, 2, 4, 6)))
    new.append(("diamond_with_a_chord", [6, 0, 4, 2], _diamond(0, 2, 4, 6) + [(2, 4)]))
    new.append(("branches_1_2_5", pu._scrambled(ev(10), 5),
                [(0, 2), (2, 18), (0, 4), (4, 6), (6, 18), (0, 8), (8, 10), (10, 12), (12, 14), (14, 16), (16, 18)]))
    new.append(("two_diamonds_sharing_a_node", ev(7), _diamond(0, 2, 4, 6) + _diamond(6, 8, 10, 12)))
    # three bubbles inside one another, each with a side branch; tails on both ends
    depth3 = [(0, 2)] + [(2, 4), (4, 26), (2, 6), (6, 8), (8, 10), (10, 22), (8, 12)] + _diamond(12, 14, 16, 18) + [(18, 20), (20, 22), (22, 24),
                                                                                                                (24, 26), (26, 28)]
    new.append(("nesting_depth_3", pu._scrambled(ev(15), 3), depth3))
    new.append(("self_loop_inside_nesting_depth_3", pu._scrambled(ev(15), 4), depth3 + [(14, 14)]))
    new.append(("nested_with_the_outer_one_discarded", ev(9), [(0, 2), (2, 2), (2, 16), (0, 4)] + _diamond(4, 6, 8, 10) + [(10, 16), (16, 14)]))
    new.append(("tip_inside", ev(5), _diamond(0, 2, 4, 6) + [(2, 8)]))
    new.append(("in_edge_from_outside", ev(5), _diamond(0, 2, 4, 6) + [(8, 2)]))
    ring = pu._ring([20, 22, 24])
    new.append(("out_edge_into_a_cycle", ev(4) + [20, 22, 24], _diamond(0, 2, 4, 6) + [(2, 20)] + ring))
    new.append(("in_edge_from_a_cycle", [20, 22, 24] + ev(4), _diamond(0, 2, 4, 6) + [(24, 2)] + ring))
    tails = [(10, 0)] + _diamond(0, 2, 4, 6) + [(6, 12)]
    for tag, x in (("entrance", 0), ("exit", 6), ("interior", 4)):
        new.append(("self_loop_on_the_" + tag, [10, 0, 2, 4, 6, 12], tails + [(x, x)]))
    new.append(("lone_self_loop", [0], [(0, 0)]))
    new.append(("self_loop_as_the_only_out_edge", [0, 2, 4, 6], [(0, 2), (2, 2), (0, 4), (4, 6)]))
    mids = ev(257, 4)
    new.append(("fan_in_257", mids + [0], [(m, 0) for m in mids]))
    new.append(("fan_out_257", [0] + mids, [(0, m) for m in mids]))
    new.append(("fan_out_and_in_257", pu._scrambled([0, 2] + mids, 257), [(0, m) for m in mids] + [(m, 2) for m in mids]))
    K = 2050   # (4 100 ranks: entrances on both sides of the prefix sum's first 4 096)
    new.append(("disjoint_edges_2050", [x for i in reversed(range(K)) for x in (4 * i + 2, 4 * i)], [(4 * i, 4 * i + 2) for i in range(K)]))
    for seed in range(10):       # sparse, local: bubbles of every kind, some nested
        rng = random.Random(100 + seed)
        ids, pairs = ev(200), set()
        for i in range(199):
            for _ in range(rng.choice((1, 1, 1, 2, 2, 3))):
                pairs.add((ids[i], ids[min(199, i + rng.choice((1, 1, 1, 2, 2, 3, 4)))]))
        new.append(("random_dag_200_seed%d" % seed, pu._scrambled(ids, seed), sorted(pairs, key=lambda e: rng.random())))
    for seed in range(5):        # the same with a few back edges (cycles) and self-loops
        rng = random.Random(200 + seed)
        ids, pairs = ev(200), set()
        for i in range(199):
            for _ in range(rng.choice((1, 1, 1, 2, 2, 3))):
                pairs.add((ids[i], ids[min(199, i + rng.choice((1, 1, 1, 2, 2, 3, 4)))]))
        for _ in range(6):
            i = rng.randrange(5, 200)
            pairs.add((ids[i], ids[i - rng.choice((0, 1, 2, 3, 5))]))
        new.append(("random_digraph_200_seed%d" % seed, pu._scrambled(ids, seed), sorted(pairs, key=lambda e: rng.random())))
    return cases + [("sb_" + name, order, edges, None) for name, order, edges in new]


# ---- golden file ---------------------------------------------------------------------------------------------------

def record_of(res):
    """The golden record of one application: the stats and the arrays, or above DIGEST_ABOVE edges their digest."""
    rec = {k: res["stats"][k] for k in STAT_KEYS}
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = cu.digest(*[res[k] for k in ARRAY_KEYS])
    else:
        for k in ARRAY_KEYS:
            rec["a_" + k] = np.asarray(res[k]).tolist()
    return rec


def check_against_record(res, rec):
    """A ``definition``-shaped result (of any producer) against one golden record."""
    assert {k: int(res["stats"][k]) for k in STAT_KEYS} == {k: rec[k] for k in STAT_KEYS}
    if "sha256" in rec:
        assert cu.digest(*[np.asarray(res[k], np.int64) for k in ARRAY_KEYS]) == rec["sha256"]
    else:
        for k in ARRAY_KEYS:
            assert np.asarray(res[k], np.int64).tolist() == list(rec["a_" + k]), k


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]
