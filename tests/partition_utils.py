"""The contract of po_layout_partition (include/phasm_overlap.h) as plain Python, the scheme the
kernels use run synchronously, the direct cases and the loader of tests/golden/partition_cases.npz.

``partition`` states the strongly connected components (Tarjan), numbered by their lowest-ranked node, the class of every
edge and the flags of every node.  ``reference_partitions`` derives from them, per weakly connected component, what the
reference's ``partition_graph`` (phasm/bubbles.py:32-84) yields, in a canonical form that does not depend on the order in
which networkx yields SCCs.  ``partition_rounds`` reaches the same SCCs the way the device does
(phasm_amd/csrc/partition.hip.h): trim rounds, forward colouring, backward marking, again while live ranks remain."""
import os
import random

import numpy as np

import components_utils as cu
import reduce_utils as ru

GOLDEN_FILE = os.path.join(ru.GOLDEN, "partition_cases.npz")
DIGEST_ABOVE = 3000      # applications with more edges keep digests of their arrays
R_IN, RE_OUT, START, SINK = 1, 2, 4, 8
R_NODE, RE_NODE = -1, -2   # 'r_' and 're_' in the canonical form
STAT_KEYS = ("n_nodes", "n_edges", "n_sccs", "n_nonsingleton_sccs", "n_singletons", "n_self_loops", "max_scc_nodes", "max_scc_edges",
             "n_class")
ARRAY_KEYS = ("node_scc", "node_flags", "edge_class", "first_node", "n_nodes", "n_edges", "n_r_in", "n_re_out")


def tarjan(n, succ):
    """root[r] = the lowest rank of r's SCC, by Tarjan's algorithm without recursion."""
    index, low, on, stack, root, counter = [-1] * n, [0] * n, [False] * n, [], [-1] * n, 0
    for s in range(n):
        if index[s] >= 0:
            continue
        work = [(s, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            descended = False
            while k < len(succ[v]):
                w = succ[v][k]
                k += 1
                if index[w] < 0:
                    work.append((v, k))
                    work.append((w, 0))
                    descended = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                for w in members:
                    root[w] = min(members)
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return root


def _ranks(edges, order):
    order = [int(x) for x in order]
    rank = {x: i for i, x in enumerate(order)}
    assert len(rank) == len(order), "a node twice in the order"
    uv = [(int(x[0]), int(x[1])) for x in edges]
    for u, v in uv:
        if u not in rank or v not in rank:
            raise ValueError("an edge has an end that is not in the node order")
    return order, [rank[u] for u, _ in uv], [rank[v] for _, v in uv]


def _result(order, eu, ev, root):
    """Everything the call returns, from the lowest rank of every rank's SCC."""
    n, m = len(order), len(eu)
    roots = sorted(set(root))
    number = {r: i for i, r in enumerate(roots)}
    node_scc = np.asarray([number[r] for r in root], dtype=np.int64)
    K = len(roots)
    n_nodes = np.bincount(node_scc, minlength=K).astype(np.int64) if n else np.zeros(0, np.int64)
    single = n_nodes == 1
    flags, cls = np.zeros(n, np.int64), np.zeros(m, np.int64)
    n_edges, indeg, outdeg = np.zeros(K, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for e, (a, b) in enumerate(zip(eu, ev)):
        ca, cb = node_scc[a], node_scc[b]
        outdeg[a] += 1
        indeg[b] += 1
        if ca == cb:
            n_edges[ca] += 1
            cls[e] = 1 if single[ca] else 0
        else:
            cls[e] = (1 if single[cb] else 2) if single[ca] else (3 if single[cb] else 4)
        if cls[e] >= 2:
            flags[a] |= RE_OUT
            flags[b] |= R_IN
    for r in range(n):
        if single[node_scc[r]]:
            flags[r] |= (START if indeg[r] == 0 else 0) | (SINK if outdeg[r] == 0 else 0)
    n_r_in = np.bincount(node_scc[(flags & R_IN) != 0], minlength=K).astype(np.int64) if n else np.zeros(0, np.int64)
    n_re_out = np.bincount(node_scc[(flags & RE_OUT) != 0], minlength=K).astype(np.int64) if n else np.zeros(0, np.int64)
    stats = {"n_nodes": n, "n_edges": m, "n_sccs": K, "n_nonsingleton_sccs": int((~single).sum()), "n_singletons": int(single.sum()),
             "n_self_loops": sum(a == b for a, b in zip(eu, ev)), "max_scc_nodes": int(n_nodes.max()) if K else 0,
             "max_scc_edges": int(n_edges.max()) if K else 0, "n_class": np.bincount(cls, minlength=5).tolist()}
    return {"node_scc": node_scc, "node_flags": flags, "edge_class": cls, "first_node": np.asarray([order[r] for r in roots], np.int64),
            "n_nodes": n_nodes, "n_edges": n_edges, "n_r_in": n_r_in, "n_re_out": n_re_out, "stats": stats}


def partition(edges, order):
    """edges: rows that start with (u, v); order: the graph's nodes in node order.  Returns ``node_scc`` and ``node_flags``
    (parallel to ``order``), ``edge_class`` (input order), per SCC ``first_node`` / ``n_nodes`` / ``n_edges`` / ``n_r_in`` /
    ``n_re_out`` and ``stats`` with the names of po_partition_stats.  An edge end outside the order raises ValueError."""
    order, eu, ev = _ranks(edges, order)
    succ = [[] for _ in order]
    for a, b in zip(eu, ev):
        succ[a].append(b)
    return _result(order, eu, ev, tarjan(len(order), succ))


def partition_rounds(edges, order):
    """The same by the device's scheme, every kernel reading the words as the kernel before left them.  ``stats`` gains
    ``n_trimmed``, ``n_outer``, the three round counts (each phase's closing round included) and ``trim_after_peel``: nodes
    trimmed in a later iteration than the first."""
    order, eu, ev = _ranks(edges, order)
    n = len(order)
    eu_, ev_ = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    proper = eu_ != ev_
    live, scc = np.ones(n, dtype=bool), np.full(n, -1, dtype=np.int64)
    w = {"n_trimmed": 0, "n_outer": 0, "n_trim_rounds": 0, "n_forward_rounds": 0, "n_backward_rounds": 0, "trim_after_peel": 0}
    while live.any():
        assert w["n_outer"] < n, "the iterations reached their cap"
        w["n_outer"] += 1
        cap, rounds = int(live.sum()) + 2, 0
        while True:
            assert rounds < cap, "the trim rounds reached their cap"
            rounds += 1
            on = proper & live[eu_] & live[ev_]
            has_out, has_in = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
            has_out[eu_[on]] = True
            has_in[ev_[on]] = True
            gone = live & ~(has_in & has_out)
            scc[gone] = np.flatnonzero(gone)
            live &= ~gone
            w["n_trimmed"] += int(gone.sum())
            w["trim_after_peel"] += int(gone.sum()) if w["n_outer"] > 1 else 0
            if not gone.any():
                break
        w["n_trim_rounds"] += rounds
        if not live.any():
            break
        cap, rounds = int(live.sum()) + 2, 0
        colour = np.where(live, np.arange(n), n)
        on = proper & live[eu_] & live[ev_]
        while True:
            assert rounds < cap, "the forward rounds reached their cap"
            rounds += 1
            before = colour.copy()
            np.minimum.at(colour, ev_[on], before[eu_[on]])
            if np.array_equal(colour, before):
                break
        w["n_forward_rounds"] += rounds
        mark, rounds = live & (colour == np.arange(n)), 0
        same = on & (colour[eu_] == colour[ev_])
        while True:
            assert rounds < cap, "the backward rounds reached their cap"
            rounds += 1
            new = np.zeros(n, dtype=bool)
            new[eu_[same & mark[ev_] & ~mark[eu_]]] = True
            mark |= new
            if not new.any():
                break
        w["n_backward_rounds"] += rounds
        assert mark.any()
        scc[mark] = colour[mark]
        live &= ~mark
    res = _result(order, eu, ev, scc.tolist())
    res["stats"].update(w)
    return res


def reference_partitions(res, weak, edges, order):
    """What ``partition_graph`` yields on every weakly connected component (``weak``: a ``components_utils.weak_components``
    result on the same input), canonically: per component the non-singleton SCCs in SCC order, then the acyclic partition.
    One dict per partition: ``component``, ``acyclic``, ``nodes`` (members in node order, then R_NODE and RE_NODE where the
    reference adds them), ``edges`` (sorted (u, v) pairs, artificial ones with R_NODE / RE_NODE), ``num_sources`` and
    ``num_sinks`` (phasm/bubbles.py:403-406)."""
    order = [int(x) for x in order]
    uv = [(int(x[0]), int(x[1])) for x in edges]
    node_scc, flags, cls = res["node_scc"], res["node_flags"], res["edge_class"]
    single = res["n_nodes"] == 1
    rank = {x: i for i, x in enumerate(order)}
    out = []
    n_comp = weak["stats"]["n_components"]
    ranks_of, edges_of = [[] for _ in range(n_comp)], [[] for _ in range(n_comp)]
    for r, c in enumerate(np.asarray(weak["node_component"]).tolist()):
        ranks_of[c].append(r)
    for e, c in enumerate(np.asarray(weak["edge_component"]).tolist()):
        edges_of[c].append(e)
    for c in range(n_comp):
        ranks, mine = ranks_of[c], edges_of[c]
        groups = [([r for r in ranks if node_scc[r] == k], [e for e in mine if cls[e] == 0 and node_scc[rank[uv[e][0]]] == k], False,
                   R_IN, RE_OUT) for k in sorted({int(node_scc[r]) for r in ranks if not single[node_scc[r]]})]
        groups.append(([r for r in ranks if single[node_scc[r]]], [e for e in mine if cls[e] == 1], True, R_IN | START, RE_OUT | SINK))
        for members, real, acyclic, in_bits, out_bits in groups:
            r_t = [order[r] for r in members if flags[r] & in_bits]
            re_s = [order[r] for r in members if flags[r] & out_bits]
            nodes = [order[r] for r in members] + ([R_NODE] if r_t else []) + ([RE_NODE] if re_s else [])
            es = sorted([uv[e] for e in real] + [(R_NODE, v) for v in r_t] + [(u, RE_NODE) for u in re_s])
            out.append({"component": c, "acyclic": acyclic, "nodes": nodes, "edges": es, "num_sources": int(bool(r_t)),
                        "num_sinks": int(bool(re_s))})
    return out


def flatten_partitions(parts):
    """The canonical partitions as integer arrays (what the golden stores and digests)."""
    return {"p_component": [p["component"] for p in parts], "p_acyclic": [int(p["acyclic"]) for p in parts],
            "p_n_nodes": [len(p["nodes"]) for p in parts], "p_n_edges": [len(p["edges"]) for p in parts],
            "p_sources": [p["num_sources"] for p in parts], "p_sinks": [p["num_sinks"] for p in parts],
            "p_nodes": [x for p in parts for x in p["nodes"]], "p_edges": [x for p in parts for e in p["edges"] for x in e]}


PART_KEYS = ("p_component", "p_acyclic", "p_n_nodes", "p_n_edges", "p_sources", "p_sinks", "p_nodes", "p_edges")


def device_partitions(parts_by_component, edges):
    """``layout.superbubble_partitions`` output in the canonical form of ``reference_partitions``."""
    uv = cu.uv_of(edges)
    out = []
    for c, parts in enumerate(parts_by_component):
        for p in parts:
            assert p.component == c and p.acyclic == (p.scc is None)
            r_t, re_s = [int(x) for x in p.r_targets], [int(x) for x in p.re_sources]
            nodes = [int(x) for x in p.nodes] + ([R_NODE] if r_t else []) + ([RE_NODE] if re_s else [])
            es = sorted([tuple(uv[e].tolist()) for e in p.edges] + [(R_NODE, v) for v in r_t] + [(u, RE_NODE) for u in re_s])
            assert (p.number_of_nodes, p.number_of_edges) == (len(nodes), len(es))
            out.append({"component": c, "acyclic": bool(p.acyclic), "nodes": nodes, "edges": es, "num_sources": p.num_sources,
                        "num_sinks": p.num_sinks})
    return out


# ---- direct cases: edges (u, v) plus an explicit node order ---------------------------------------------------------------

def _path(nodes):
    return list(zip(nodes, nodes[1:]))


def _ring(nodes):
    return _path(nodes) + [(nodes[-1], nodes[0])]


def _scrambled(nodes, seed):
    out = list(nodes)
    random.Random(seed).shuffle(out)
    return out


def direct_inputs():
    """(name, order, edges, n_ids or None).  Nodes are even ids; ``n_ids`` is given where ids at or above it name merged
    nodes."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    cases = [("empty", [], [], None), ("nodes_without_edges", [4, 2, 0], [], None), ("one_self_loop_alone", [0], [(0, 0)], None),
             ("self_loop_with_an_in_edge", [0, 2], [(0, 2), (2, 2)], None), ("two_cycle", [2, 0], [(0, 2), (2, 0)], None),
             ("three_cycle_with_tails", [0, 2, 4, 6, 8], [(0, 2)] + _ring([2, 4, 6]) + [(6, 8)], None),
             ("two_cycles_sharing_a_node", [2, 0, 4], [(0, 2), (2, 0), (0, 4), (4, 0)], None),
             ("two_cycles_joined_by_an_edge", [0, 2, 4, 6], [(0, 2), (2, 0), (2, 4), (4, 6), (6, 4)], None)]
    # cycle -> bridge -> cycle, the bridge's first node ranked lowest: it colours what lies downstream
    a, b = [2, 4, 6], [20, 22, 24]
    cases.append(("cycle_bridge_cycle", [0] + a + b, _ring(a) + [(6, 0), (0, 20)] + _ring(b), None))
    bridge = [0, 10, 12, 14]
    cases.append(("cycle_bridge_path_cycle", bridge[:1] + a + b + bridge[1:], _ring(a) + [(6, 0)] + _path(bridge) + [(14, 20)] + _ring(b), None))
    cycles = [ev(3, 6 * i) for i in range(6)]
    chain = [e for c in cycles for e in _ring(c)] + [(cycles[i][2], cycles[i + 1][0]) for i in range(5)]
    cases.append(("six_cycles_ascending", [x for c in cycles for x in c], chain, None))
    cases.append(("six_cycles_descending", [x for c in reversed(cycles) for x in c], chain, None))
    cases.append(("every_node_in_a_cycle", [0, 2, 4, 6, 8], _ring([0, 2, 4]) + [(6, 8), (8, 6)], None))
    k8 = ev(8)
    cases.append(("k8_both_directions", k8, [(u, v) for u in k8 for v in k8 if u != v], None))
    ids = ev(1025)
    for tag, order in (("ascending", ids), ("descending", ids[::-1]), ("scrambled", _scrambled(ids, 1025))):
        cases.append(("path_1025_" + tag, order, _path(ids), None))
    for n in (257, 1025):
        ids = ev(n)
        for tag, order in (("ascending", ids), ("scrambled", _scrambled(ids, n))):
            cases.append(("ring_%d_%s" % (n, tag), order, _ring(ids), None))
    K = 2050   # (4 100 ranks: roots on both sides of the prefix sum's first 4 096)
    cases.append(("two_cycles_2050", [x for i in reversed(range(K)) for x in (4 * i, 4 * i + 2)],
                  [e for i in range(K) for e in ((4 * i, 4 * i + 2), (4 * i + 2, 4 * i))], None))
    cases.append(("merged_ids", [9, 0, 8, 3, 10, 6], [(8, 0), (0, 8), (3, 9), (10, 10), (9, 8), (8, 6)], 8))
    for k, (m, seed) in enumerate([(300, 1), (500, 2), (300, 3), (500, 4), (300, 5), (500, 6), (300, 7), (500, 8), (300, 9), (500, 10)]):
        rng = random.Random(seed)
        ids = ev(200)
        pairs = set()
        while len(pairs) < m:
            pairs.add((rng.choice(ids), rng.choice(ids)))
        cases.append(("random_200_%d_seed%d" % (m, seed), _scrambled(ids, seed), sorted(pairs, key=lambda e: rng.random()), None))
    return cases


# ---- golden file ---------------------------------------------------------------------------------------------------

def by_uv(edges):
    e = cu.uv_of(edges)
    return np.lexsort((e[:, 1], e[:, 0]))


def record_of(res, parts, edges):
    """The golden record of one application: the arrays of ``partition`` (``edge_class`` in (u, v) order) and the canonical
    partitions, or above DIGEST_ABOVE edges their digests."""
    rec = {k: res["stats"][k] for k in STAT_KEYS}
    arrays = {k: np.asarray(res[k]) for k in ARRAY_KEYS}
    arrays["edge_class"] = arrays["edge_class"][by_uv(edges)]
    flat = flatten_partitions(parts)
    rec["n_partitions"] = len(parts)
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = cu.digest(*[arrays[k] for k in ARRAY_KEYS])
        rec["partitions_sha256"] = cu.digest(*[flat[k] for k in PART_KEYS])
    else:
        for k in ARRAY_KEYS:
            rec["a_" + k] = arrays[k].tolist()
        rec.update(flat)
    return rec


def check_against_record(res, parts, edges, rec):
    """A ``partition``-shaped result and canonical partitions (of any producer) against one golden record."""
    got = dict(res["stats"])
    got["n_class"] = [int(x) for x in got["n_class"]]
    assert {k: got[k] for k in STAT_KEYS} == {k: rec[k] for k in STAT_KEYS}
    arrays = {k: np.asarray(res[k], dtype=np.int64) for k in ARRAY_KEYS}
    arrays["edge_class"] = arrays["edge_class"][by_uv(edges)]
    flat = flatten_partitions(parts)
    assert len(parts) == rec["n_partitions"]
    if "sha256" in rec:
        assert cu.digest(*[arrays[k] for k in ARRAY_KEYS]) == rec["sha256"]
        assert cu.digest(*[flat[k] for k in PART_KEYS]) == rec["partitions_sha256"]
    else:
        for k in ARRAY_KEYS:
            assert arrays[k].tolist() == list(rec["a_" + k]), k
        for k in PART_KEYS:
            assert list(flat[k]) == list(rec[k]), k


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]
