"""The contract of po_phase_paths (include/phasm_overlap.h) as plain Python, the scheme the kernels use
run synchronously in numpy, the direct cases and the loader of tests/golden/paths_cases.npz.

``definition`` takes the top-level bubbles, their chains and their interiors from ``superbubble_utils.scheme`` and
``bubblechain_utils.scheme`` (min_nodes 1), counts the paths of a bubble by a memoised sum over the successors and lists them
by a depth-first walk that takes the successors in edge order.  ``scheme`` reaches the same the way the device does
(phasm_amd/csrc/paths.hip.h): the edges sorted by (tail rank, edge index), counting rounds in which a member sums its
successors once an earlier round has finished them all, one walk per listed path that unranks its index through the counts,
the interior by a sort of (bubble, rank)."""
import os
import sys

import numpy as np

import bubblechain_utils as bu
import components_utils as cu
import partition_utils as pu
import reduce_utils as ru
import superbubble_utils as su

GOLDEN_FILE = os.path.join(ru.GOLDEN, "paths_cases.npz")
BARE, UNLISTED, SATURATED = 1, 2, 4
MANY = 2**64 - 1
MAX_LISTED, MAX_NODES = 2**30, 2**31
TABLE_KEYS = ("b_entrance", "b_exit", "b_chain", "b_position", "b_inside", "b_flags", "b_paths", "b_path_nodes")
CSR_KEYS = ("inside_off", "inside_nodes", "pred_off", "pred_node", "pred_weight", "bubble_path_off", "path_off", "path_nodes")
ARRAY_KEYS = TABLE_KEYS + CSR_KEYS
STAT_KEYS = ("n_nodes", "n_edges", "n_bubbles", "n_bare", "n_unlisted", "n_saturated", "n_listed_paths", "n_path_nodes", "max_paths_seen",
             "max_path_nodes", "n_stray_edges")


class Capacity(Exception):
    """What the call refuses with PO_ERR_CAPACITY."""


def sat_add(a, b):
    return min(a + b, MANY)


def _bubbles(edges, order):
    """(order, eu, ev, weight, [(entrance rank, exit rank, chain, position, sorted interior ranks)] by (chain, position))."""
    order, eu, ev = pu._ranks(edges, order)
    order = [int(x) for x in order]
    rank = {x: r for r, x in enumerate(order)}
    e = np.asarray(edges, dtype=np.int64).reshape(len(edges), -1) if len(edges) else np.zeros((0, 3), np.int64)
    weight = e[:, 2].tolist() if e.shape[1] > 2 else [0] * len(e)
    sb = su.scheme(edges, order)
    bc = bu.scheme(edges, order, 1, sb)
    sets = su.node_sets(sb, order)
    out = []
    for i, nested in enumerate(sb["b_nested"].tolist()):
        if nested:
            continue
        s, t = rank[int(sb["b_entrance"][i])], rank[int(sb["b_exit"][i])]
        assert bc["node_chain"][s] != bu.NONE, "with min_nodes 1 every top-level bubble lies in a chain"
        out.append((s, t, int(bc["node_chain"][s]), int(bc["node_bubble"][s]), sorted(rank[x] for x in sets[i] if rank[x] not in (s, t))))
        assert len(out[-1][4]) == int(sb["b_inside"][i])
    out.sort(key=lambda b: (b[2], b[3]))
    return order, [int(x) for x in eu], [int(x) for x in ev], weight, out


def _finish(order, n_edges, rows, csr, n_stray, extra=None):
    """Everything the call returns from the per-bubble rows (s, t, chain, position, n_inside, flags, n_paths, n_path_nodes)."""
    res = {k: np.asarray([r[i] for r in rows], dtype=np.uint64 if k == "b_paths" else np.int64) for i, k in enumerate(TABLE_KEYS)}
    for k in CSR_KEYS:
        res[k] = np.asarray(csr[k], dtype=np.int64)
    flags, lens = res["b_flags"], np.diff(res["path_off"])
    res["stats"] = {"n_nodes": len(order), "n_edges": n_edges, "n_bubbles": len(rows), "n_bare": int((flags & BARE != 0).sum()),
                    "n_unlisted": int((flags & UNLISTED != 0).sum()), "n_saturated": int((flags & SATURATED != 0).sum()),
                    "n_listed_paths": len(res["path_off"]) - 1, "n_path_nodes": len(res["path_nodes"]),
                    "max_paths_seen": max([int(r[6]) for r in rows] + [0]), "max_path_nodes": int(lens.max()) if len(lens) else 0,
                    "n_stray_edges": n_stray}
    res["stats"].update(extra or {})
    return res


def _flags(n_inside, n_paths, max_paths):
    sat = n_paths == MANY
    return (BARE if n_inside == 0 else 0) | (UNLISTED if sat or n_paths > max_paths else 0) | (SATURATED if sat else 0)


# ---- the definition ---------------------------------------------------------------------------------------------------------

def definition(edges, order, max_paths):
    """edges: rows that start with (u, v[, weight]); order: the graph's nodes in node order.  Returns the table columns
    ``b_*`` by (chain, position), the CSR arrays and ``stats`` with the names of po_paths_stats.  Raises ``Capacity`` where the
    call refuses."""
    order, eu, ev, weight, bubbles = _bubbles(edges, order)
    n = len(order)
    succ, pred = [[] for _ in range(n)], [[] for _ in range(n)]
    for k, (a, b) in enumerate(zip(eu, ev)):
        succ[a].append(b)                      # (the edge order is the adjacency order)
        pred[b].append((a, k))
    rows, n_stray, listed = [], 0, 0
    csr = {k: [0] if k.endswith("_off") else [] for k in CSR_KEYS}
    todo = []
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    for s, t, chain, position, interior in bubbles:
        inside, cnt = set(interior), {t: 1}

        def count(v):
            if v not in cnt:
                cnt[v] = 0                     # (a cycle cannot occur; the word keeps the recursion finite if one did)
                total = 0
                for w in succ[v]:
                    total = sat_add(total, count(w) if w == t or w in inside else 0)
                cnt[v] = total
            return cnt[v]

        n_paths = count(s)
        n_stray += sum(1 for v in [s] + interior for w in succ[v] if w != t and w not in inside)
        flags = _flags(len(interior), n_paths, max_paths)
        listed += 0 if flags & UNLISTED else n_paths
        todo.append((s, t, inside, flags))
        rows.append([order[s], order[t], chain, position, len(interior), flags, n_paths, 0])
        csr["inside_nodes"] += [order[v] for v in interior]
        csr["inside_off"].append(len(csr["inside_nodes"]))
        for p, k in pred[t]:
            csr["pred_node"].append(order[p])
            csr["pred_weight"].append(weight[k])
        csr["pred_off"].append(len(csr["pred_node"]))
    if listed >= MAX_LISTED:
        raise Capacity("paths")
    for row, (s, t, inside, flags) in zip(rows, todo):
        first = len(csr["path_nodes"])
        if not flags & UNLISTED:
            stack = [(s, [s])]                 # depth first, the successors in order: networkx.all_simple_paths on a DAG
            while stack:
                v, path = stack.pop()
                if v == t:
                    csr["path_nodes"] += [order[x] for x in path]
                    csr["path_off"].append(len(csr["path_nodes"]))
                    continue
                for w in reversed(succ[v]):
                    if w == t or w in inside:
                        stack.append((w, path + [w]))
        row[7] = len(csr["path_nodes"]) - first
        csr["bubble_path_off"].append(len(csr["path_off"]) - 1)
    if len(csr["path_nodes"]) >= MAX_NODES:
        raise Capacity("nodes")
    return _finish(order, len(eu), rows, csr, n_stray)


# ---- the device's scheme, run synchronously -------------------------------------------------------------------------------------

def scheme(edges, order, max_paths):
    """The same by the device's scheme; ``stats`` gains ``n_count_rounds`` (the closing round included; 0 without a bubble)."""
    order, eu, ev, weight, bubbles = _bubbles(edges, order)
    n, m = len(order), len(eu)
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    home, bidx, exit_of, n_inside = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for b, (s, t, _, _, interior) in enumerate(bubbles):
        home[s], bidx[s], exit_of[s], n_inside[s] = s, b, t, len(interior)
        home[interior] = s
    # the edges of the members by (tail, edge index): first and one-past-last place of every tail
    member_tail = home[eu] >= 0 if m else np.zeros(0, bool)
    key = np.sort(np.where(member_tail, (eu << 32) | np.arange(m), -1).astype(np.uint64)) if m else np.zeros(0, np.uint64)
    first, last = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tails = (key >> np.uint64(32)).astype(np.int64)
    for i in range(m):
        if key[i] == np.uint64(MANY):
            break
        if i == 0 or tails[i - 1] != tails[i]:
            first[tails[i]] = i
        if i + 1 == m or tails[i + 1] != tails[i]:
            last[tails[i]] = i + 1
    heads = [int(ev[int(k) & 0xFFFFFFFF]) if k != np.uint64(MANY) else -1 for k in key]
    inside_w = lambda w, s: w != s and home[w] == s   # noqa: E731
    n_stray = sum(1 for a, b in zip(eu.tolist(), ev.tolist()) if home[a] >= 0 and b != exit_of[home[a]] and not inside_w(b, home[a]))
    # the counting rounds: a word written in this round is "not yet"
    cnt, done = [0] * n, [0] * n
    rounds, cap = 0, (max([len(b[4]) for b in bubbles]) if bubbles else 0) + 2
    while bubbles:
        rounds += 1
        assert rounds <= cap, "the counting rounds reached their bound"
        wrote = []
        for v in range(n):
            s = home[v]
            if s < 0 or done[v]:
                continue
            t, total, ready = exit_of[s], 0, True
            for i in range(first[v], last[v]):
                w = heads[i]
                if w == t:
                    total = sat_add(total, 1)
                elif inside_w(w, s):
                    if not 0 < done[w] < rounds:
                        ready = False
                        break
                    total = sat_add(total, cnt[w])
            if ready:
                wrote.append((v, total))
        for v, total in wrote:
            cnt[v], done[v] = total, rounds
        if not wrote:
            break
    rows, listed = [], 0
    csr = {k: [0] if k.endswith("_off") else [] for k in CSR_KEYS}
    exits = {b[1] for b in bubbles}
    pred_key = sorted((b, k) for k, b in enumerate(ev.tolist()) if b in exits)      # (head rank, edge index) of the in-edges of exits
    in_edges = {}
    for b, k in pred_key:
        in_edges.setdefault(b, []).append(k)
    for s, t, chain, position, interior in bubbles:
        flags = _flags(len(interior), cnt[s], max_paths)
        listed += 0 if flags & UNLISTED else min(cnt[s], 0x7FFFFFFF)
        rows.append([order[s], order[t], chain, position, len(interior), flags, cnt[s], 0])
        for k in in_edges.get(t, []):
            csr["pred_node"].append(order[int(eu[k])])
            csr["pred_weight"].append(weight[k])
        csr["pred_off"].append(len(csr["pred_node"]))
    if listed >= MAX_LISTED:
        raise Capacity("paths")
    # the interior: (bubble << 32 | rank) sorted
    ikey = sorted((int(bidx[home[r]]) << 32) | r for r in range(n) if home[r] >= 0 and home[r] != r)
    csr["inside_nodes"] = [order[k & 0xFFFFFFFF] for k in ikey]
    csr["inside_off"] = [0] + np.cumsum([len(b[4]) for b in bubbles]).tolist()
    # one walk per listed path
    for row, (s, t, _, _, interior) in zip(rows, bubbles):
        first_node = len(csr["path_nodes"])
        for j in range(0 if row[5] & UNLISTED else row[6]):
            v, path = s, [s]
            for _ in range(len(interior) + 1):
                for i in range(first[v], last[v]):
                    w = heads[i]
                    c = 1 if w == t else (cnt[w] if inside_w(w, s) else 0)
                    if j < c:
                        break
                    j -= c
                else:
                    raise AssertionError("no successor holds the path")
                path.append(w)
                v = w
                if w == t:
                    break
            assert path[-1] == t, "a walk did not reach its exit within n_inside + 1 steps"
            csr["path_nodes"] += [order[x] for x in path]
            csr["path_off"].append(len(csr["path_nodes"]))
        row[7] = len(csr["path_nodes"]) - first_node
        csr["bubble_path_off"].append(len(csr["path_off"]) - 1)
    if len(csr["path_nodes"]) >= MAX_NODES:
        raise Capacity("nodes")
    return _finish(order, m, rows, csr, n_stray, {"n_count_rounds": rounds})


def result_of(bp, stats=None):
    """A ``phasm_amd.phasing.BubblePaths`` in the form of ``definition``."""
    t = bp.bubbles
    res = {"b_entrance": t["entrance"], "b_exit": t["exit"], "b_chain": t["chain"], "b_position": t["position"], "b_inside": t["n_inside"],
           "b_flags": t["flags"], "b_path_nodes": t["n_path_nodes"]}
    res = {k: np.asarray(v, dtype=np.int64) for k, v in res.items()}
    res["b_paths"] = np.asarray(t["n_paths"], dtype=np.uint64)
    for k in CSR_KEYS:
        res[k] = np.asarray(getattr(bp, k)).astype(np.int64)
    res["stats"] = dict(stats or {})
    return res


def same(got, want, stats=True):
    for k in ARRAY_KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k][:20], want[k][:20])
    if stats:
        assert {k: got["stats"][k] for k in STAT_KEYS} == {k: want["stats"][k] for k in STAT_KEYS}


# ---- the direct cases -----------------------------------------------------------------------------------------------------------

def first_seen(edges):
    """The nodes in the order in which add_edge first sees them."""
    order = []
    for e in edges:
        for x in e[:2]:
            if x not in order:
                order.append(x)
    return order


def _w(edges):
    """A weight per edge that tells the edges apart."""
    return [(u, v, 1000 + 7 * k) for k, (u, v) in enumerate(edges)]


def diamonds_in_series(k, first=0):
    """x0 -> (a_i | b_i) -> x_{i+1}, k times: nodes first .. first + 3k; 2^k paths from x0 to xk."""
    edges, x = [], first
    for _ in range(k):
        edges += [(x, x + 1), (x, x + 2), (x + 1, x + 3), (x + 2, x + 3)]
        x += 3
    return edges, x


def many_paths(k):
    """s -> x0, k diamonds in series, xk -> t, plus s -> z -> t: 2^k + 1 paths."""
    inner, last = diamonds_in_series(k, 2)
    s, t, z = 0, last + 1, 1
    return [(s, 2)] + inner + [(last, t), (s, z), (z, t)]


def direct_inputs():
    """(name, order, edges with weights, max_paths)."""
    out = []

    def add(name, edges, max_paths, order=None):
        edges = _w(edges)
        out.append((name, list(order) if order is not None else first_seen(edges), edges, max_paths))

    for name, order, edges, n_ids in su.direct_inputs():
        if name.startswith(("sb_", "merged_ids", "random_200_300_seed1")) and "1025" not in name and "2050" not in name:
            add("su_" + name, [tuple(e) for e in edges], 16, order)
    # a bubble with a nested bubble inside a nested bubble
    add("nested_in_nested", [(0, 1), (1, 2), (2, 3), (2, 4), (3, 5), (4, 5), (5, 6), (1, 7), (7, 6), (6, 8), (0, 9), (9, 8), (8, 10)], 16)
    # an exit with in-degree 1, 2 and 65
    add("exit_in_degree_1", [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)], 16)
    add("exit_in_degree_2", [(0, 1), (0, 2), (1, 3), (2, 3)], 16)
    add("exit_in_degree_65", [(0, 1 + i) for i in range(65)] + [(1 + i, 66) for i in range(65)], 100)
    # one graph under three permutations of its edge list
    base = [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4), (1, 5), (3, 5), (4, 6), (5, 6), (2, 6), (6, 7), (6, 8), (7, 9), (8, 9)]
    for k in range(3):
        perm = np.random.default_rng(40 + k).permutation(len(base)) if k else np.arange(len(base))
        add("permuted_%d" % k, [base[i] for i in perm], 16, order=list(range(10)))
    # the direct edge s -> t first, in the middle and last among the successors of s
    arms = [(0, 1), (0, 2), (1, 3), (2, 3)]
    add("direct_edge_first", [(0, 3)] + arms, 16, order=[0, 1, 2, 3])
    add("direct_edge_middle", [(0, 1), (0, 3), (0, 2), (1, 3), (2, 3)], 16, order=[0, 1, 2, 3])
    add("direct_edge_last", arms + [(0, 3)], 16, order=[0, 1, 2, 3])
    # a chain that ends in a bare bubble with bubbles behind it; two chains in one graph
    d1, a = diamonds_in_series(2)
    d2, b = diamonds_in_series(2, a + 1)
    add("bare_in_the_middle", d1 + [(a, a + 1)] + d2, 16)
    d3, c = diamonds_in_series(3, b + 5)
    add("two_chains", d1 + [(a, a + 1)] + d2 + d3, 16)
    # a bubble of exactly max_paths and one of max_paths + 1
    add("exactly_max_paths", many_paths(3), 9)
    add("max_paths_plus_one", many_paths(3), 8)
    add("counts_only", many_paths(3), 0)
    # 2^64 + 1 paths: saturated; 2^62 + 1: not saturated, unlisted
    add("saturated_64", many_paths(64), 1000)
    add("unlisted_62", many_paths(62), 1000)
    # more than one wave of paths in one bubble: 7 diamonds in series and an arm, 129 paths
    add("one_bubble_129_paths", many_paths(7), 200)
    return out


# ---- disjoint unions of golden cases: sizes past one grid at the price of the small cases ---------------------------------------

UNION_NAMES = ("direct_one_bubble_129_paths", "direct_two_chains", "direct_nested_in_nested", "direct_permuted_1")


def union_of(cases, copies, layout):
    """Disjoint copies of the cases' graphs: (node order, edges, expected result).  copy_major: copy after copy; interleaved:
    node i of every copy, then node i + 1, the edges likewise -- inside a copy the relative order of nodes and of edges is the
    case's own, so every copy keeps the case's result (node ids shifted); the chains are numbered by the rank of their heads."""
    items, shift = [], 0
    for c in range(copies):
        for case in cases:
            order, edges, max_paths = case_inputs(case)
            items.append((shift, np.asarray(order, np.int64), np.asarray(edges, np.int64).reshape(-1, 3), result_of_record(case["result"])))
            shift += (max(order) | 1) + 1

    def lay(arrays):
        if layout == "copy_major":
            return np.concatenate(arrays)
        longest = max(len(a) for a in arrays)
        idx = np.concatenate([np.arange(len(a)) for a in arrays])
        return np.concatenate(arrays)[np.argsort(idx, kind="stable")] if longest else np.concatenate(arrays)

    order = lay([o + s for s, o, _, _ in items])
    edges = lay([e + np.asarray([s, s, 0]) for s, _, e, _ in items])
    rank_of = np.full(shift, -1, np.int64)
    rank_of[order] = np.arange(len(order))
    keys, segs = [], []
    for i, (s, _, _, r) in enumerate(items):
        head = {}
        for b in range(len(r["b_entrance"])):
            if r["b_position"][b] == 0:
                head[int(r["b_chain"][b])] = int(r["b_entrance"][b])
        for b in range(len(r["b_entrance"])):
            keys.append((int(rank_of[head[int(r["b_chain"][b])] + s]), int(r["b_position"][b])))
            segs.append((i, b))
    by = sorted(range(len(keys)), key=keys.__getitem__)
    heads = sorted({k[0] for k in keys})
    chain_of = {h: j for j, h in enumerate(heads)}
    cols = {k: [] for k in TABLE_KEYS}
    parts = {k: [] for k in ("inside_nodes", "pred_node", "pred_weight", "path_nodes", "path_len")}
    for j in by:
        i, b = segs[j]
        s, _, _, r = items[i]
        for k in TABLE_KEYS:
            cols[k].append(int(r[k][b]))
        cols["b_entrance"][-1] += s
        cols["b_exit"][-1] += s
        cols["b_chain"][-1] = chain_of[keys[j][0]]
        parts["inside_nodes"].append(r["inside_nodes"][r["inside_off"][b]:r["inside_off"][b + 1]] + s)
        parts["pred_node"].append(r["pred_node"][r["pred_off"][b]:r["pred_off"][b + 1]] + s)
        parts["pred_weight"].append(r["pred_weight"][r["pred_off"][b]:r["pred_off"][b + 1]])
        p0, p1 = int(r["bubble_path_off"][b]), int(r["bubble_path_off"][b + 1])
        parts["path_nodes"].append(r["path_nodes"][r["path_off"][p0]:r["path_off"][p1]] + s)
        parts["path_len"].append(np.diff(r["path_off"][p0:p1 + 1]))
    cat = lambda k: np.concatenate(parts[k]) if parts[k] else np.zeros(0, np.int64)   # noqa: E731
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)   # noqa: E731
    want = {k: np.asarray(v, dtype=np.uint64 if k == "b_paths" else np.int64) for k, v in cols.items()}
    want.update({"inside_nodes": cat("inside_nodes"), "pred_node": cat("pred_node"), "pred_weight": cat("pred_weight"),
                 "path_nodes": cat("path_nodes"), "inside_off": off([len(x) for x in parts["inside_nodes"]]),
                 "pred_off": off([len(x) for x in parts["pred_node"]]), "bubble_path_off": off([len(x) for x in parts["path_len"]]),
                 "path_off": off(cat("path_len"))})
    return order, edges, want


# ---- golden file ------------------------------------------------------------------------------------------------------------------

def record_of(res):
    rec = {k: res[k].tolist() for k in ARRAY_KEYS if k != "b_paths"}
    rec["b_paths"] = [str(int(x)) for x in res["b_paths"]]       # (up to 2^64 - 1: as text)
    rec["stats"] = {k: (str(v) if k == "max_paths_seen" else v) for k, v in res["stats"].items() if k in STAT_KEYS + ("n_count_rounds",)}
    return rec


def result_of_record(rec):
    res = {k: np.asarray(rec[k], dtype=np.int64) for k in ARRAY_KEYS if k != "b_paths"}
    res["b_paths"] = np.asarray([int(x) for x in rec["b_paths"]], dtype=np.uint64)
    res["stats"] = {k: (int(v) if k == "max_paths_seen" else v) for k, v in rec["stats"].items()}
    return res


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]


def case_inputs(c):
    """(order, edges as [n, 3] rows, max_paths) of a golden case."""
    return list(c["order"]), np.asarray(c["edges_flat"], dtype=np.int64).reshape(-1, 3).tolist(), int(c["max_paths"])
