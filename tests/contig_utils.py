"""The contract of po_layout_contigs (include/phasm_overlap.h) as plain Python, the scheme the kernels
use run synchronously, the direct cases and the loader of tests/golden/contig_cases.npz.

``definition`` restates the reference's sequential queue walk (identify_contigs, phasm/assembly_graph.py:655-718) with its
``visited_edges`` set: the initial queue of the edges whose first node has in-degree 0 or above 1, the extension loop, the
edges queued at a branch point, the nodes without edges.  ``scheme`` reaches the same the way the device does
(phasm_amd/csrc/contigs.hip.h): the class of every edge, list ranking of the extensions toward their head edge, a second
ranking over the heads for the coverage of the late starts, the sums at the heads, the filter, the numbering.

A graph here is ``edges`` -- rows (u, v, weight) -- with ``order``, its nodes in node order; ``lengths`` maps a node to its
length, ``exclude`` is a set of nodes."""
import os
from collections import deque

import numpy as np

import components_utils as cu
import partition_utils as pu
import reduce_utils as ru

GOLDEN_FILE = os.path.join(ru.GOLDEN, "contig_cases.npz")
DIGEST_ABOVE = pu.DIGEST_ABOVE
NONE = -1
ARRAY_KEYS = ("edge_contig", "edge_pos", "c_first", "c_last", "c_nodes", "c_first_edge", "c_length")
STAT_KEYS = ("n_nodes", "n_edges", "n_excluded", "n_root_starts", "n_late_starts", "n_blocked", "n_covered_edges", "n_uncovered_edges",
             "n_paths", "n_short_paths", "n_isolated", "n_short_isolated", "n_contigs", "max_path_nodes")
SCHEME_KEYS = ("n_path_rounds", "n_cover_rounds", "max_path_depth", "max_cover_depth")


def _inputs(edges, order, lengths, exclude):
    order, eu, ev = pu._ranks(edges, order)
    n = len(order)
    w = np.asarray([int(x[2]) for x in edges], np.int64)
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    nlen = np.asarray([int(lengths[x]) for x in order], np.int64)
    excl = np.asarray([x in exclude for x in order], bool)
    indeg = np.bincount(ev, minlength=n) if n else np.zeros(0, np.int64)
    outdeg = np.bincount(eu, minlength=n) if n else np.zeros(0, np.int64)
    return order, eu, ev, w, nlen, excl, indeg, outdeg


def _result(order, eu, ev, w, nlen, excl, indeg, outdeg, paths, min_len):
    """Everything the call returns.  paths: the edge lists of EVERY path (head edge first), covered and not dropped yet."""
    n, m = len(order), len(eu)
    start = indeg[eu] != 1 if m else np.zeros(0, bool)
    late = (~start) & (outdeg[eu] > 1) if m else np.zeros(0, bool)
    blocked = (start | late) & excl[eu] & excl[ev] if m else np.zeros(0, bool)
    length_of = lambda p: int(w[p].sum()) + int(nlen[ev[p[-1]]])   # noqa: E731
    paths = sorted(paths, key=lambda p: (int(eu[p[0]]), p[0]))     # numbered by (rank of the first node, head edge)
    kept = [p for p in paths if length_of(p) >= min_len]
    edge_contig, edge_pos = np.full(m, NONE, np.int64), np.full(m, NONE, np.int64)
    seen = np.zeros(m, bool)
    for p in paths:
        assert not seen[p].any(), "an edge lies on two paths"
        seen[p] = True
    for j, p in enumerate(kept):
        edge_contig[p], edge_pos[p] = j, np.arange(len(p))
    iso = [r for r in range(n) if indeg[r] == 0 and outdeg[r] == 0]
    iso_kept = [r for r in iso if nlen[r] >= min_len]
    stats = {"n_nodes": n, "n_edges": m, "n_excluded": int(excl.sum()), "n_root_starts": int(start.sum()), "n_late_starts": int(late.sum()),
             "n_blocked": int(blocked.sum()), "n_covered_edges": int(seen.sum()), "n_uncovered_edges": m - int(seen.sum()),
             "n_paths": len(paths), "n_short_paths": len(paths) - len(kept), "n_isolated": len(iso),
             "n_short_isolated": len(iso) - len(iso_kept), "n_contigs": len(kept) + len(iso_kept),
             "max_path_nodes": max([len(p) + 1 for p in paths] + [0])}
    arr = lambda a: np.asarray(a, np.int64)   # noqa: E731
    return {"edge_contig": edge_contig, "edge_pos": edge_pos,
            "c_first": arr([order[eu[p[0]]] for p in kept] + [order[r] for r in iso_kept]),
            "c_last": arr([order[ev[p[-1]]] for p in kept] + [order[r] for r in iso_kept]),
            "c_nodes": arr([len(p) + 1 for p in kept] + [1] * len(iso_kept)),
            "c_first_edge": arr([p[0] for p in kept] + [NONE] * len(iso_kept)),
            "c_length": arr([length_of(p) for p in kept] + [int(nlen[r]) for r in iso_kept]), "stats": stats}


# ---- the reference's walk -------------------------------------------------------------------------------------------------

def definition(edges, order, lengths, exclude=(), min_contig_len=5000):
    """The queue walk of identify_contigs on ranks and edge indices.  Returns ``edge_contig`` / ``edge_pos`` parallel to
    ``edges`` (NONE where there is none), the table ``c_first`` / ``c_last`` / ``c_nodes`` / ``c_first_edge`` / ``c_length`` in
    contig order, ``stats``."""
    order, eu, ev, w, nlen, excl, indeg, outdeg = _inputs(edges, order, lengths, set(exclude))
    n = len(order)
    out_edges = [[] for _ in range(n)]
    for e, u in enumerate(eu.tolist()):
        out_edges[u].append(e)
    both = lambda e: excl[eu[e]] and excl[ev[e]]   # noqa: E731
    queue = deque(e for u in range(n) for e in out_edges[u] if (indeg[u] == 0 or indeg[u] > 1) and not both(e))
    visited, paths = set(), []
    while queue:
        e = queue.popleft()
        if e in visited:
            continue
        visited.add(e)
        path = [e]
        outgoing = out_edges[ev[e]]
        while len(outgoing) == 1:
            oe = outgoing[0]
            if oe in visited:
                break
            if indeg[eu[oe]] > 1:
                break
            path.append(oe)
            visited.add(oe)
            outgoing = out_edges[ev[oe]]
        paths.append(path)
        outgoing = out_edges[ev[path[-1]]]
        if len(outgoing) > 1:
            for oe in outgoing:
                if both(oe):
                    continue
                if oe not in visited:
                    queue.append(oe)
    assert sum(len(p) for p in paths) == len(visited)
    return _result(order, eu, ev, w, nlen, excl, indeg, outdeg, paths, min_contig_len)


# ---- the device's scheme, run synchronously -------------------------------------------------------------------------------

def scheme(edges, order, lengths, exclude=(), min_contig_len=5000):
    """The same by the device's scheme; ``stats`` gains the round counts of the two pointer-jumping loops (closing rounds
    included; 0 where the graph has no edge), the most edges between an edge and the head it reached, and the most heads
    between a late start and the final head it reached."""
    order, eu, ev, w, nlen, excl, indeg, outdeg = _inputs(edges, order, lengths, set(exclude))
    n, m = len(order), len(eu)
    if m == 0:
        res = _result(order, eu, ev, w, nlen, excl, indeg, outdeg, [], min_contig_len)
        res["stats"].update({"n_path_rounds": 0, "n_cover_rounds": 0, "max_path_depth": 0, "max_cover_depth": 0})
        return res
    ine = np.full(n, NONE, np.int64)
    ine[ev] = np.arange(m)                                   # (read only where the in-degree is 1)
    start = indeg[eu] != 1
    late = (~start) & (outdeg[eu] > 1)
    is_start = start | late
    blocked = is_start & excl[eu] & excl[ev]
    idx = np.arange(m, dtype=np.int64)
    # list ranking of the extensions toward their head: hops += hops[jb]; jb = jb[jb]; done = the link names a start
    jb = np.where(is_start, idx, ine[eu])
    done = is_start | is_start[jb]
    hops, ws = (~is_start).astype(np.int64), np.where(is_start, 0, w)
    path_rounds = 0
    while True:
        assert path_rounds < m + 2, "the ranking rounds reached their cap"
        path_rounds += 1
        go = ~done
        jj, dj = jb[jb], done[jb]
        resolved = int((go & dj).sum())
        hops, ws = np.where(go, hops + hops[jb], hops), np.where(go, ws + ws[jb], ws)       # (a ring's sums wrap: never read)
        jb, done = np.where(go, jj, jb), done | (go & dj)
        if not resolved:
            break
    head = np.where(done, jb, NONE)                          # the head edge of every edge that reached one
    # coverage of the late starts: ok &= ok[cj]; cj = cj[cj] over the heads; final = a root start or a dead late start
    parent = np.where(late, head[ine[eu]], NONE)             # the head of the path that ends at the first node
    dead = late & (parent == NONE)
    final = start | dead
    ok = np.where(is_start, ~blocked & ~dead, False)
    cj = np.where(late & ~dead, parent, idx)
    cdone = final | (late & ~dead & final[cj])
    ok = np.where(late & ~dead & final[cj], ok & ok[cj], ok)
    depth = np.where(cdone, 1, 0)
    cover_rounds = 0
    while True:
        assert cover_rounds < m + 2, "the coverage rounds reached their cap"
        cover_rounds += 1
        go = is_start & ~cdone
        cc, dc = cj[cj], cdone[cj]
        resolved = int((go & dc).sum())
        ok = np.where(go, ok & ok[cj], ok)
        cj, cdone = np.where(go, cc, cj), cdone | (go & dc)
        if not resolved:
            break
    covered_head = is_start & cdone & ok
    covered = np.where(head != NONE, covered_head[np.maximum(head, 0)], False)
    # the deepest late start that reached a final head, in heads above it (a statistic for the round bound)
    max_depth = 0
    for s in np.flatnonzero(late & cdone).tolist():
        d, x = 0, s
        while not final[x]:
            x, d = int(parent[x]), d + 1
        max_depth = max(max_depth, d)
    paths = {int(h): [None] * 0 for h in np.flatnonzero(covered_head).tolist()}
    place = {}
    for e in np.flatnonzero(covered).tolist():
        place.setdefault(int(head[e]), {})[0 if is_start[e] else int(hops[e])] = e
    out = []
    for h in paths:
        p = place[h]
        assert sorted(p) == list(range(len(p))), "the places of a path have a gap"
        edges_of = [p[k] for k in range(len(p))]
        last = edges_of[-1]
        assert not (indeg[ev[last]] == 1 and outdeg[ev[last]] == 1), "a path ends where it could go on"
        total = int(w[h]) + (0 if last == h else int(ws[last]))
        assert total == int(w[edges_of].sum())
        out.append(edges_of)
    res = _result(order, eu, ev, w, nlen, excl, indeg, outdeg, out, min_contig_len)
    res["stats"].update({"n_path_rounds": path_rounds, "n_cover_rounds": cover_rounds,
                         "max_path_depth": int(hops[done].max()) if done.any() else 0, "max_cover_depth": max_depth})
    return res


def log2_ceil(x):
    return max(int(x) - 1, 0).bit_length()


def round_bounds(stats):
    """ceil(log2(longest)) + 1, the closing round included, for (the ranking rounds, the coverage rounds): an entry d links
    from its root is resolved after k rounds iff d <= 2^k, and the first round that resolves nothing is the last."""
    return log2_ceil(max(stats["max_path_depth"], 1)) + 1, log2_ceil(max(stats["max_cover_depth"], 1)) + 1


def path_of(res, edges, j):
    """The node ids of contig ``j`` in path order."""
    if res["c_first_edge"][j] == NONE:
        return [int(res["c_first"][j])]
    on = sorted((int(res["edge_pos"][e]), e) for e in np.flatnonzero(res["edge_contig"] == j).tolist())
    return [int(edges[on[0][1]][0])] + [int(edges[e][1]) for _, e in on]


def paths_of(res, edges):
    return [tuple(path_of(res, edges, j)) for j in range(len(res["c_first"]))]


# ---- direct cases ---------------------------------------------------------------------------------------------------------

def _weights(uv, seed):
    rng = np.random.default_rng(seed)
    return [(int(u), int(v), int(x)) for (u, v), x in zip(uv, rng.integers(1, 400, len(uv)))]


def direct_inputs():
    """(name, order, edges (u, v, weight), lengths {node: length}, exclude (sorted list), min_contig_len).  Nodes are even ids
    (oriented reads of the + strand); lengths are 100 + node unless a case is about them."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    L = lambda nodes: {int(x): 100 + int(x) for x in nodes}   # noqa: E731
    cases = []
    add = lambda name, order, edges, lengths=None, exclude=(), min_len=0: cases.append(   # noqa: E731
        (name, [int(x) for x in order], [tuple(int(y) for y in e) for e in edges], lengths or L(order), sorted(int(x) for x in exclude),
         int(min_len)))
    add("empty", [], [])
    ids = ev(1025)
    zig = [ids[i // 2] if i % 2 == 0 else ids[-1 - i // 2] for i in range(len(ids))]
    for tag, order in (("identity", ids), ("reversed", ids[::-1]), ("scrambled", pu._scrambled(ids, 1025)), ("zigzag", zig)):
        add("path_1025_" + tag, order, _weights(pu._path(ids), 5))
    big = 2**31 - 1
    add("weight_sum_above_2_to_32", ev(4), [(0, 2, big), (2, 4, big - 1), (4, 6, big - 2)], min_len=2**32)
    add("weight_sum_below_a_64_bit_minimum", ev(4), [(0, 2, big), (2, 4, big - 1), (4, 6, big - 2)], min_len=3 * big + 200)
    for m in (40, 1025):
        add("ring_%d" % m, pu._scrambled(ev(m), m), _weights(pu._ring(ev(m)), m))
    # a tail into a ring: the ring's path starts at the junction (in-degree 2) and ends at it
    add("lasso", pu._scrambled(ev(12), 3), _weights(pu._path(ev(5)) + pu._path(ev(8, 8)) + [(22, 8)], 1))
    # a ring of in-degree-1 nodes with a spur out: the late starts at the branch are never reached
    add("ring_with_a_spur_out", ev(9), _weights(pu._ring(ev(6)) + [(4, 12), (12, 14), (14, 16)], 2))
    # 300 late starts in a row: a spine 0 -> 2 -> 4 ..., every spine node with a tooth
    spine = ev(301)
    teeth = [(spine[i], 1000 + 2 * i) for i in range(300)]
    add("comb_300", pu._scrambled(spine + [t for _, t in teeth], 300), _weights(pu._path(spine) + teeth, 300))
    tree = [(2 * i, 2 * (2 * i + 1)) for i in range(1023)] + [(2 * i, 2 * (2 * i + 2)) for i in range(1023)]
    add("binary_out_tree_depth_10", pu._scrambled(ev(2047), 10), _weights(tree, 10))
    small_tree = [(0, 2), (2, 4), (2, 6), (4, 8), (4, 10), (6, 12)]
    add("blocked_root_start_with_a_tree_behind", ev(7), _weights(small_tree, 3), exclude=[0, 2])
    add("blocked_late_start_beside_an_open_sibling", ev(7), _weights(small_tree, 3), exclude=[2, 4])
    add("path_through_a_stretch_of_excluded_nodes", ev(8), _weights(pu._path(ev(8)), 4), exclude=[4, 6, 8])
    add("every_node_excluded", ev(8), _weights(pu._path(ev(8)), 4), exclude=ev(8))
    add("self_loop_as_head_edge", ev(4), _weights([(0, 2), (2, 2), (2, 4), (4, 6)], 6))
    add("self_loop_on_an_in_degree_1_node", ev(4), _weights([(2, 2), (2, 4), (4, 6)], 6))
    add("two_cycle_entered_from_outside", ev(3), _weights([(0, 2), (2, 4), (4, 2)], 7))
    add("isolated_nodes_at_and_below_the_minimum", [8, 0, 2, 4, 6], [(0, 2, 10)], {0: 5, 2: 5, 4: 60, 6: 59, 8: 61}, min_len=60)
    add("minimum_0_reports_everything_covered", [8, 0, 2, 4, 6], [(0, 2, 0), (2, 4, -5)], {0: 0, 2: 0, 4: 0, 6: 0, 8: 0}, min_len=0)
    add("negative_length_is_below_every_minimum", ev(3), [(0, 2, -500), (2, 4, 7)], L(ev(3)), min_len=0)
    K = 2050
    order = [x for i in reversed(range(K)) for x in (4 * i + 2, 4 * i)]
    add("pairs_2050_scrambled", pu._scrambled(order, K), _weights([(4 * i, 4 * i + 2) for i in range(K)], K), min_len=300)
    for seed in range(6):
        rng = np.random.default_rng(1000 + seed)
        n = 200
        m = int(n * (0.8 + 0.14 * seed))
        pairs = set()
        while len(pairs) < m:
            u, v = rng.integers(0, n, 2)
            pairs.add((2 * int(u), 2 * int(v)))
        nodes = pu._scrambled(ev(n), seed)
        excl = [x for x in nodes if rng.random() < 0.3]
        add("random_200_seed_%d" % seed, nodes, _weights(sorted(pairs), seed), {x: int(rng.integers(0, 300)) for x in nodes}, excl,
            (0, 150, 400)[seed % 3])
    return cases


# ---- golden file ---------------------------------------------------------------------------------------------------

def _canonical(res, edges):
    """The arrays of a result with the edge arrays in the order of the edges sorted by (u, v) and ``c_first_edge`` as that
    order's index: what a record holds, whatever order the producer's graph keeps its edges in (a graph has no edge twice).
    The numbering of the contigs depends on the edge order only among heads that leave the same node; a record keeps the
    contigs sorted by (first node's place in the table, (u, v) of the head edge), so it does not."""
    e = cu.uv_of(edges)
    m = len(e)
    by = np.lexsort((e[:, 1], e[:, 0])) if m else np.zeros(0, np.int64)
    place = np.empty(m, np.int64)
    place[by] = np.arange(m)
    fe = np.asarray(res["c_first_edge"], np.int64)
    fe_c = np.where(fe != NONE, place[np.maximum(fe, 0)] if m else fe, NONE)
    k = len(fe)
    # contigs that share a first node are consecutive in the table: order each such run by the canonical head edge
    first = np.asarray(res["c_first"], np.int64)
    run = np.zeros(k, np.int64)
    if k:
        run[1:] = np.cumsum((first[1:] != first[:-1]) | (fe[1:] == NONE) | (fe[:-1] == NONE))
    perm = np.lexsort((fe_c, run)) if k else np.zeros(0, np.int64)
    new_of = np.empty(k, np.int64)
    new_of[perm] = np.arange(k)
    ec = np.asarray(res["edge_contig"], np.int64)
    ec = np.where(ec != NONE, new_of[np.maximum(ec, 0)] if k else ec, NONE)
    out = {"edge_contig": ec[by], "edge_pos": np.asarray(res["edge_pos"], np.int64)[by], "c_first_edge": fe_c[perm]}
    for key in ("c_first", "c_last", "c_nodes", "c_length"):
        out[key] = np.asarray(res[key], np.int64)[perm]
    return [out[key] for key in ARRAY_KEYS]


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
