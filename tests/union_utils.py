"""Graphs made of disjoint copies of small cases, and the rules by which the result of a graph stage on such a union follows
from its result on one copy.  Plain numpy, no device.

Every graph stage treats weakly connected components independently, so a union of R disjoint copies has, per copy, exactly
the single case's answer.  That gives an expectation at 600 000+ items that costs one run of the CPU definitions on the
small case: tests/test_union_rules.py proves the rules on the CPU (definition on the union == broadcast of the definition on
one copy), tests/test_gpu_union_scale.py holds the device to the broadcast at sizes past one capped grid and one scan
window.

A union is built from K cases and a list that says which case every copy is.  Copy c gets its node ids shifted by the ids
of the copies before it (``base[c]``) and its segment names suffixed with ``.c``.  Two layouts:

* ``copy_major``:  all lines of copy 0, then copy 1, ...: ids keep their locality;
* ``interleaved``: line i of every copy in turn, then line i + 1: the edges of one node lie far apart and the node order
  alternates between the copies.

The rules:

* per edge and per node (flags, kept edges, classes, component / SCC / exit / chain / contig, place): the single copy's value,
  node ids shifted by ``base[c]``, table indices renumbered as below;
* tables (merged paths, components, SCCs, superbubbles, chains, contigs): the entries of all copies, numbered by the rank of
  their head node in the union's node order -- (introducing line, copy, slot) when interleaved, (copy, rank in copy) when
  copy-major;
* counters: additive ones are the sum over the copies, maxima the maximum; round counts are not additive and no rule is
  given for them.  One counter is neither: the superbubble stage's ``n_p_nodes`` counts the two virtual nodes 'r_' and 're_'
  once per graph, not once per copy (``virtual_nodes``)."""
import numpy as np

LAYOUTS = ("copy_major", "interleaved")
NONE = -1


def i64(a, width=None):
    a = np.asarray(a, dtype=np.int64)
    return a.reshape(-1, width) if width else a


class Union:
    def __init__(self, n_ids, copies, layout):
        """n_ids[k]: the node ids case k takes (even: two per segment); copies[c]: the case of copy c."""
        assert layout in LAYOUTS
        self.n_ids = i64(n_ids)
        assert (self.n_ids % 2 == 0).all()
        self.case_of = i64(copies)
        self.R = len(self.case_of)
        self.layout = layout
        width = self.n_ids[self.case_of]
        self.base = np.cumsum(width) - width
        self.total_ids = int(width.sum())

    # ---- sequences: lines, edges, node orders, table entries -------------------------------------------------------
    def gather(self, per_case, copy, idx):
        """per_case[case of copy][idx], for arrays of (copy, idx)."""
        case = self.case_of[copy]
        first = i64(per_case[0])
        out = np.empty((len(copy),) + first.shape[1:], dtype=np.int64)
        for k, a in enumerate(per_case):
            m = case == k
            if m.any():
                out[m] = i64(a).reshape((-1,) + first.shape[1:])[idx[m]]
        return out

    def sequence(self, keys, layout=None):
        """The union of one sequence per copy.  keys[k]: for every item of case k's sequence the line that holds it,
        non-decreasing (a list of lines: its own index).  Returns (copy, idx) per item of the union: copy after copy, or
        sorted by (line, copy, place in the copy's sequence)."""
        n = i64([len(k) for k in keys])[self.case_of]
        start = np.cumsum(n) - n
        copy = np.repeat(np.arange(self.R, dtype=np.int64), n)
        idx = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(start, n)
        if (layout or self.layout) == "interleaved":
            o = np.lexsort((idx, copy, self.gather(keys, copy, idx)))
            copy, idx = copy[o], idx[o]
        return copy, idx

    def lines(self, counts):
        return self.sequence([np.arange(n) for n in counts])

    def place(self, seq, counts):
        """(where, start): item idx of copy c stands at where[start[c] + idx] in the union sequence ``seq``."""
        copy, idx = seq
        n = i64(counts)[self.case_of]
        start = np.cumsum(n) - n
        where = np.full(int(n.sum()), NONE, dtype=np.int64)
        where[start[copy] + idx] = np.arange(len(copy))
        return where, start

    # ---- ids ---------------------------------------------------------------------------------------------------------
    def shift(self, nodes, copy, none=NONE):
        nodes = i64(nodes)
        return np.where(nodes == none, none, nodes + self.base[copy])

    def locate(self, nodes):
        """(copy, id inside the copy) of union node ids below ``total_ids``."""
        nodes = i64(nodes)
        copy = np.searchsorted(self.base, nodes, side="right") - 1
        return copy, nodes - self.base[copy]

    def locate_edges(self, uv, per_case_uv):
        """(copy, index in its case's edge list) of every union edge (u, v): an edge list of the union in any order."""
        uv = i64(uv, 2) if len(uv) else np.zeros((0, 2), np.int64)
        copy, lu = self.locate(uv[:, 0])
        copy_v, lv = self.locate(uv[:, 1])
        assert (copy == copy_v).all(), "an edge joins two copies"
        idx = np.full(len(uv), NONE, dtype=np.int64)
        case = self.case_of[copy]
        for k, e in enumerate(per_case_uv):
            e = i64(e).reshape(len(e), -1) if len(e) else np.zeros((0, 2), np.int64)
            key = e[:, 0] * self.n_ids[k] + e[:, 1]
            o = np.argsort(key, kind="stable")
            m = case == k
            want = lu[m] * self.n_ids[k] + lv[m]
            at = np.searchsorted(key[o], want)
            assert len(key) or not m.any()
            at = np.minimum(at, max(len(key) - 1, 0))
            assert (key[o][at] == want).all(), "an edge that no copy has"
            idx[m] = o[at]
        return copy, idx

    # ---- tables -------------------------------------------------------------------------------------------------------
    def table(self, head_rank, node_place, groups=None):
        """The union of one table per copy, numbered by the rank of each entry's head node.  head_rank[k]: the rank, in case
        k's node order, of the head node of every entry; node_place: ``place`` of the union's node order; groups[k]: a major
        key per entry (contigs: paths before one-node contigs).  Entries of one copy with the same head keep their order.
        Returns (copy, idx) per union entry and (number, start): entry idx of copy c is number[start[c] + idx]."""
        where, nstart = node_place
        copy, idx = self.sequence([np.arange(len(h)) for h in head_rank], layout="copy_major")
        rank = where[nstart[copy] + self.gather(head_rank, copy, idx)] if len(copy) else np.zeros(0, np.int64)
        group = self.gather(groups, copy, idx) if groups is not None and len(copy) else np.zeros(len(copy), np.int64)
        o = np.lexsort((idx, rank, group))
        seq = (copy[o], idx[o])
        return seq, self.place(seq, [len(h) for h in head_rank])

    @staticmethod
    def renumber(values, copy, numbering, none=NONE):
        number, start = numbering
        values = i64(values)
        safe = np.where(values == none, 0, values)
        return np.where(values == none, none, number[np.minimum(start[copy] + safe, max(len(number) - 1, 0))] if len(number) else none)


def rank_array(order, n_ids):
    r = np.full(n_ids, NONE, dtype=np.int64)
    r[i64(order)] = np.arange(len(order))
    return r


# ---- building unions ---------------------------------------------------------------------------------------------------

def row_union(cases, copies, layout):
    """cases: (names, lengths, rows) as the generators of the utils give them.  Returns the union and its segment names,
    segment lengths, rows and the (copy, line) of every row."""
    U = Union([2 * len(c[1]) for c in cases], copies, layout)
    seq = U.lines([len(c[2]) for c in cases])
    rows = U.gather([i64(c[2], 6) for c in cases], *seq)
    rows[:, 0] += U.base[seq[0]]
    rows[:, 1] += U.base[seq[0]]
    lengths = np.concatenate([i64(cases[k][1]) for k in U.case_of.tolist()]) if U.R else np.zeros(0, np.int64)
    return U, lengths, rows, seq


def union_names(cases, U):
    return ["%s.%d" % (n, c) for c, k in enumerate(U.case_of.tolist()) for n in cases[k][0]]


def gfa_text(cases, U, seq):
    """GFA2 text of a row union: the S lines copy after copy (segment i of copy c is segment base[c] / 2 + i of the file),
    then the E lines in the union's layout.  One string template per case line, one substitution per copy."""
    seg, edge = [], []
    for names, lengths, rows in cases:
        seg.append("".join("S\t%s.@\t%d\t*\n" % (n, l) for n, l in zip(names, lengths)))
        edge.append("".join("E\t*\t%s.@%s\t%s.@%s\t%d\t%d\t%d\t%d\t*\n" % (names[a >> 1], "+-"[a & 1], names[b >> 1], "+-"[b & 1], s, e, bs, be)
                            for a, b, s, e, bs, be in i64(rows, 6).tolist()))
    out = ["H\tVN:z:2.0\n"] + [seg[k].replace("@", str(c)) for c, k in enumerate(U.case_of.tolist())]
    per_copy = [edge[k].replace("@", str(c)).splitlines(True) for c, k in enumerate(U.case_of.tolist())]
    flat = np.empty(sum(len(x) for x in per_copy), dtype=object)
    flat[:] = [l for x in per_copy for l in x]
    where, start = U.place(U.sequence([np.arange(len(c[2])) for c in cases], layout="copy_major"), [len(c[2]) for c in cases])
    out += flat[where[start[seq[0]] + seq[1]]].tolist()
    return "".join(out)


def graph_union(cases, copies, layout, width=4):
    """cases: (order, edges) with edges (u, v, ...) of ``width`` columns.  Returns the union, its edges, its node order and
    the (copy, idx) of both."""
    n_ids = [(max([int(x) for x in order] + [int(y) for e in edges for y in e[:2]] + [-1]) | 1) + 1 for order, edges in cases]
    U = Union(n_ids, copies, layout)
    eseq = U.lines([len(e) for _, e in cases])
    nseq = U.lines([len(o) for o, _ in cases])
    edges = U.gather([i64(e, width) if len(e) else np.zeros((0, width), np.int64) for _, e in cases], *eseq)
    edges[:, 0] += U.base[eseq[0]]
    edges[:, 1] += U.base[eseq[0]]
    order = U.gather([i64(o) for o, _ in cases], *nseq) + U.base[nseq[0]]
    return U, edges, order, eseq, nseq


# ---- the rules -------------------------------------------------------------------------------------------------------------

def node_order(U, orders, intro_rows):
    """The union's node order from each case's node order and the row that brought each node in (tips_utils.node_order with
    ``with_rows``): (nodes, (copy, idx))."""
    seq = U.sequence([i64(r) for r in intro_rows])
    return U.gather([i64(o) for o in orders], *seq) + U.base[seq[0]], seq


def stage1_edges(U, per_case_edges):
    """The union's stage-1 edges sorted by (u, v): the shifts grow with the copy, so that is copy after copy."""
    srt = [i64(e, 4)[np.lexsort((i64(e, 4)[:, 1], i64(e, 4)[:, 0]))] if len(e) else np.zeros((0, 4), np.int64) for e in per_case_edges]
    copy, idx = U.sequence([np.arange(len(e)) for e in srt], layout="copy_major")
    out = U.gather(srt, copy, idx)
    out[:, 0] += U.base[copy]
    out[:, 1] += U.base[copy]
    return out


def add_stats(U, stats, add, maxima=()):
    """Counters of the union: ``add`` keys summed over the copies (lists element by element), ``maxima`` keys their maximum."""
    n = np.bincount(U.case_of, minlength=len(stats))
    out = {}
    for k in add:
        vals = [np.asarray(s[k], dtype=np.int64) * int(c) for s, c in zip(stats, n)]
        tot = sum(vals)
        out[k] = tot.tolist() if np.ndim(tot) else int(tot)
    for k in maxima:
        out[k] = max([int(s[k]) for s, c in zip(stats, n) if c] + [0])
    return out


def per_item(U, per_case, seq, kind="plain", numbering=None):
    """One array of the union from the same array of every case, along the union sequence ``seq``: plain values, node ids
    (shifted) or table indices (renumbered)."""
    v = U.gather(per_case, *seq) if len(seq[0]) else np.zeros(0, np.int64)
    if kind == "node":
        return U.shift(v, seq[0])
    if kind == "table":
        return U.renumber(v, seq[0], numbering)
    return v


def broadcast(U, spec, singles, orders, nseq, eseq):
    """The result of a graph-analysis stage on the union from its results on the cases.  spec: {"node": {key: kind}, "edge":
    {key: kind}, "table": {key: kind}, "head": the table column with the head node, "group": None or a function of a single
    result giving a major key per entry, "add": additive counters, "max": maxima}; kinds: "plain", "node", "table", "edge".
    nseq / eseq: (copy, idx) of the union's node order and edges."""
    ranks = [rank_array(o, int(n)) for o, n in zip(orders, U.n_ids)]
    nplace = U.place(nseq, [len(o) for o in orders])
    eplace = U.place(eseq, [len(s[next(iter(spec["edge"]))]) if spec["edge"] else 0 for s in singles]) if spec["edge"] else None
    head = [r[i64(s[spec["head"]])] if len(s[spec["head"]]) else np.zeros(0, np.int64) for r, s in zip(ranks, singles)]
    groups = [i64(spec["group"](s)) for s in singles] if spec.get("group") else None
    tseq, numbering = U.table(head, nplace, groups)
    out = {}
    for where, seq in (("node", nseq), ("edge", eseq), ("table", tseq)):
        for key, kind in spec[where].items():
            if kind == "edge":
                v = U.gather([s[key] for s in singles], *seq) if len(seq[0]) else np.zeros(0, np.int64)
                out[key] = U.renumber(v, seq[0], eplace)
            else:
                out[key] = per_item(U, [s[key] for s in singles], seq, kind, numbering)
    out["stats"] = add_stats(U, [s["stats"] for s in singles], spec["add"], spec["max"])
    return out


COMPONENTS = {"node": {"node_component": "table"}, "edge": {"edge_component": "table"},
              "table": {"first_node": "node", "n_nodes": "plain", "n_edges": "plain"}, "head": "first_node",
              "add": ("n_nodes", "n_edges", "n_components", "n_singletons"), "max": ("max_component_nodes", "max_component_edges")}
PARTITION = {"node": {"node_scc": "table", "node_flags": "plain"}, "edge": {"edge_class": "plain"},
             "table": {"first_node": "node", "n_nodes": "plain", "n_edges": "plain", "n_r_in": "plain", "n_re_out": "plain"},
             "head": "first_node", "add": ("n_nodes", "n_edges", "n_sccs", "n_nonsingleton_sccs", "n_singletons", "n_self_loops", "n_class"),
             "max": ("max_scc_nodes", "max_scc_edges")}
SUPERBUBBLES = {"node": {"node_exit": "node", "node_inside": "node", "node_flags": "plain"}, "edge": {},
                "table": {"b_entrance": "node", "b_exit": "node", "b_inside": "plain", "b_nested": "plain"}, "head": "b_entrance",
                "add": ("n_nodes", "n_edges", "n_p_edges", "n_bubbles", "n_nested", "n_self_loop_nodes", "n_discarded"), "max": ()}
BUBBLECHAINS = {"node": {"node_chain": "table", "node_bubble": "plain"}, "edge": {"edge_chain": "table"},
                "table": {"c_first": "node", "c_last": "node", "c_bubbles": "plain", "c_nodes": "plain", "c_edges": "plain"}, "head": "c_first",
                "add": ("n_nodes", "n_edges", "n_bubbles", "n_top", "n_chains", "n_short", "n_chain_nodes", "n_chain_edges"),
                "max": ("max_chain_bubbles",)}
CONTIGS = {"node": {}, "edge": {"edge_contig": "table", "edge_pos": "plain"},
           "table": {"c_first": "node", "c_last": "node", "c_nodes": "plain", "c_first_edge": "edge", "c_length": "plain"}, "head": "c_first",
           "group": lambda s: i64(s["c_first_edge"]) == NONE,
           "add": ("n_nodes", "n_edges", "n_excluded", "n_root_starts", "n_late_starts", "n_blocked", "n_covered_edges", "n_uncovered_edges",
                   "n_paths", "n_short_paths", "n_isolated", "n_short_isolated", "n_contigs"), "max": ("max_path_nodes",)}


def virtual_nodes(partition_result):
    """(has 'r_', has 're_') of one graph: superbubble_utils._structure counts each once in ``n_p_nodes``."""
    single = (i64(partition_result["n_nodes"]) == 1)[i64(partition_result["node_scc"])] if len(partition_result["node_scc"]) else np.zeros(0, bool)
    f = i64(partition_result["node_flags"])
    return int((single & ((f & (1 | 4)) != 0)).any()), int((single & ((f & (2 | 8)) != 0)).any())


def superbubble_p_nodes(U, singles, virtuals):
    """``n_p_nodes`` of the union: the real nodes add up, each virtual node is there once if any copy has it."""
    n = np.bincount(U.case_of, minlength=len(singles))
    real = sum(int(c) * (s["stats"]["n_p_nodes"] - a - b) for s, (a, b), c in zip(singles, virtuals, n))
    return real + max([a for (a, _), c in zip(virtuals, n) if c] + [0]) + max([b for (_, b), c in zip(virtuals, n) if c] + [0])


def edge_flags(U, per_case_flags, located):
    """Per-edge values of an edge-list stage along the union's edges (located by ``locate_edges``)."""
    return per_item(U, per_case_flags, located)


def order_left(U, order, nseq, per_case_left, orders):
    """The node order a cleaning stage leaves: the union's order without the nodes their copy dropped."""
    alive = [np.isin(i64(o), i64(l)) for o, l in zip(orders, per_case_left)]
    return i64(order)[U.gather([a.astype(np.int64) for a in alive], *nseq) != 0] if len(order) else i64(order)


def merged(U, singles, orders, nseq, located):
    """The result of merge_utils.merge_paths on the union from the cases' results (each on its own edges in any fixed order,
    merged node k written as the case's n_ids + k).  located: (copy, idx) of the union's input edges; nseq: (copy, idx) of its
    node order.  Merged node j of the union is ``total_ids + j``, numbered by the rank of its head."""
    ranks = [rank_array(o, int(n)) for o, n in zip(orders, U.n_ids)]
    nplace = U.place(nseq, [len(o) for o in orders])
    heads = [r[i64(s["members"])[i64(s["offsets"])[:-1]]] if len(s["lengths"]) else np.zeros(0, np.int64) for r, s in zip(ranks, singles)]
    (pcopy, pidx), numbering = U.table(heads, nplace)

    def ids(v, copy):
        """node ids of a copy's result in the union: reads shifted, merged nodes renumbered"""
        v = i64(v)
        n = U.n_ids[U.case_of[copy]]
        is_merged = v >= n
        return np.where(is_merged, U.total_ids + U.renumber(np.where(is_merged, v - n, 0), copy, numbering), v + U.base[copy])

    flags = per_item(U, [s["flags"] for s in singles], located)
    kept_at = [np.cumsum(i64(s["flags"]) != 1) - 1 for s in singles]                 # place among the kept edges
    keep = flags != 1
    kcopy, kidx = located[0][keep], U.gather(kept_at, *located)[keep] if len(flags) else np.zeros(0, np.int64)
    edges = U.gather([i64(s["edges"], 4) if len(s["edges"]) else np.zeros((0, 4), np.int64) for s in singles], kcopy, kidx) \
        if keep.any() else np.zeros((0, 4), np.int64)
    if len(edges):
        edges[:, 0], edges[:, 1] = ids(edges[:, 0], kcopy), ids(edges[:, 1], kcopy)
    # the order: the nodes that are on no path, then the merged nodes
    on_path = [np.isin(i64(o), i64(s["members"])).astype(np.int64) for o, s in zip(orders, singles)]
    order = (U.gather([i64(o) for o in orders], *nseq) + U.base[nseq[0]])[U.gather(on_path, *nseq) == 0] if len(nseq[0]) else np.zeros(0, np.int64)
    order = np.concatenate([order, U.total_ids + np.arange(len(pcopy))])
    # the tables, path after path
    n_members = [np.diff(i64(s["offsets"])) for s in singles]
    plen = U.gather(n_members, pcopy, pidx) if len(pcopy) else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)
    first = U.gather([i64(s["offsets"])[:-1] for s in singles], pcopy, pidx) if len(pcopy) else np.zeros(0, np.int64)
    mcopy = np.repeat(pcopy, plen)
    at = np.repeat(first, plen) + np.arange(int(plen.sum())) - np.repeat(offsets[:-1], plen)
    members = U.gather([s["members"] for s in singles], mcopy, at) + U.base[mcopy] if len(at) else np.zeros(0, np.int64)
    prefix = U.gather([s["prefix"] for s in singles], mcopy, at) if len(at) else np.zeros(0, np.int64)
    lengths = U.gather([s["lengths"] for s in singles], pcopy, pidx) if len(pcopy) else np.zeros(0, np.int64)
    stats = add_stats(U, [s["stats"] for s in singles],
                      ("n_edges_in", "n_edges_out", "n_nodes", "n_merged", "n_nodes_merged", "n_self_loops", "n_cycle_nodes", "n_overflow", "n_invalid"),
                      ("max_path_nodes",))
    return {"flags": flags, "edges": edges, "order": order, "offsets": offsets, "members": members, "prefix": prefix, "lengths": lengths,
            "stats": stats, "kept": (kcopy, kidx)}


# ---- the stages that start from rows: one case (or a union itself) through the CPU definitions ----------------------------

FUZZ, TIP_L, TIP_B = 1000, 4, 5000


def row_pipeline(lengths, rows):
    """Every stage that takes rows or a stage-1 result, by the CPU definitions the goldens pin, on one set of rows (segment
    lengths, rows).  Edge arrays are in the order the reference's graph first saw the edges."""
    import coverage_utils as cu
    import diamond_utils as du
    import merge_utils as mu
    import reduce_utils as ru
    import tips_utils as tu
    from oracle import layout_oracle as lo
    L = np.repeat(i64(lengths), 2)
    rows = i64(rows, 6) if len(rows) else np.zeros((0, 6), np.int64)
    seq = lo.layout_sequential(rows.tolist(), L.tolist())
    s1 = i64([(u, v, w, o) for (u, v), (w, o) in seq["edges"].items()], 4) if seq["edges"] else np.zeros((0, 4), np.int64)
    contained = np.zeros(len(L) // 2, dtype=np.int64)
    contained[[n >> 1 for n in seq["filters"][0]["nodes_to_remove"]]] = 1
    order, intro = tu.node_order(rows.tolist(), L.tolist(), with_rows=True)
    P = {"n_ids": len(L), "L": L, "rows": rows, "s1": s1, "contained": contained, "order": i64(order), "intro": i64(intro),
         "stage1_stats": {"n_rows": len(rows), "n_type": [seq["types"].count(t) for t in range(4)], "n_contained_reads": int(contained.sum()),
                          "n_edges": len(s1)}}
    f = ru.reduce_edges(s1, FUZZ)
    P["reduce"] = {"flags": i64(f), "stats": {"n_edges_in": len(s1), "n_transitive": int((f == 1).sum()), "n_asymmetric": int((f == 2).sum()),
                                              "n_edges_out": int((f == 0).sum()),
                                              "max_out_degree": int(np.bincount(s1[:, 0]).max()) if len(s1) else 0}}
    f, left, st = tu.remove_tips(s1, order, TIP_L, TIP_B)
    P["tips"] = {"flags": i64(f), "left": i64(left), "stats": st}
    f, left, st = du.remove_diamond_tips(s1, order)
    P["diamonds"] = {"flags": i64(f), "left": i64(left), "stats": st}
    removed_by, e_final, order_final, stats4 = du.clean_chain(s1, order, FUZZ, TIP_L, TIP_B, reduce_flags=P["reduce"]["flags"])
    P["chain"] = {"removed_by": i64(removed_by), "left": i64(order_final), "stats": stats4}
    P["merge"] = mu.merge_paths(s1, order, L.tolist())
    P["merge"]["order"] = i64(P["merge"]["order"])
    for key, graph in (("coverage", s1), ("coverage_merged", P["merge"]["edges"])):
        members, lengths_all = None, L
        if key == "coverage_merged":
            m = P["merge"]
            members = {len(L) + k: m["members"][m["offsets"][k]:m["offsets"][k + 1]].tolist() for k in range(len(m["lengths"]))}
            lengths_all = np.concatenate([L, m["lengths"]])
        sums, paths, _ = cu.edge_coverage(rows, graph, members, lengths_all) if len(graph) else (np.zeros(0, np.int64),) * 3
        n_nodes, n_pairs, max_set = cu.set_stats(rows, graph, members)
        P[key] = {"read_length_sum": sums, "path_length": paths,
                  "stats": {"n_edges": len(graph), "n_rows": len(rows), "n_nodes": n_nodes, "n_pairs": n_pairs, "max_set": max_set}}
    return P


TIPS_ADD = ("n_edges_in", "n_in_tip_edges", "n_out_tip_edges", "n_asymmetric", "n_edges_out", "n_nodes", "n_isolated_nodes", "n_candidates_in",
            "n_candidates_out")
DIAMOND_ADD = ("n_edges_in", "n_edges_out", "n_nodes", "n_nodes_removed", "n_candidates", "n_diamonds", "n_invalid")
REDUCE_ADD = ("n_edges_in", "n_transitive", "n_asymmetric", "n_edges_out")
COVERAGE_ADD = ("n_edges", "n_rows", "n_nodes", "n_pairs")


def row_expectation(U, Ps, s1_union):
    """What ``row_pipeline`` (or the device) must give on the union, from its results ``Ps`` on the cases.  s1_union: the
    union's stage-1 edges in the order the per-edge arrays are wanted in (the producer's own: a graph has no edge order)."""
    s1_union = i64(s1_union, 4) if len(s1_union) else np.zeros((0, 4), np.int64)
    located = U.locate_edges(s1_union[:, :2], [P["s1"][:, :2] for P in Ps])
    orders = [P["order"] for P in Ps]
    order, nseq = node_order(U, orders, [P["intro"] for P in Ps])
    W = {"s1_sorted": stage1_edges(U, [P["s1"] for P in Ps]), "order": order, "located": located, "nseq": nseq,
         "contained": np.concatenate([Ps[k]["contained"] for k in U.case_of.tolist()]) if U.R else np.zeros(0, np.int64),
         "stage1_stats": add_stats(U, [P["stage1_stats"] for P in Ps], ("n_rows", "n_type", "n_contained_reads", "n_edges"))}
    W["reduce"] = {"flags": edge_flags(U, [P["reduce"]["flags"] for P in Ps], located),
                   "stats": add_stats(U, [P["reduce"]["stats"] for P in Ps], REDUCE_ADD, ("max_out_degree",))}
    for key, add in (("tips", TIPS_ADD), ("diamonds", DIAMOND_ADD)):
        W[key] = {"flags": edge_flags(U, [P[key]["flags"] for P in Ps], located),
                  "left": order_left(U, order, nseq, [P[key]["left"] for P in Ps], orders),
                  "stats": add_stats(U, [P[key]["stats"] for P in Ps], add)}
    W["chain"] = {"removed_by": edge_flags(U, [P["chain"]["removed_by"] for P in Ps], located),
                  "left": order_left(U, order, nseq, [P["chain"]["left"] for P in Ps], orders),
                  "stats": [add_stats(U, [P["chain"]["stats"][i] for P in Ps], add)
                            for i, add in enumerate((REDUCE_ADD, TIPS_ADD, DIAMOND_ADD, TIPS_ADD))]}
    W["merge"] = merged(U, [P["merge"] for P in Ps], orders, nseq, located)
    W["coverage"] = {k: per_item(U, [P["coverage"][k] for P in Ps], located) for k in ("read_length_sum", "path_length")}
    W["coverage"]["stats"] = add_stats(U, [P["coverage"]["stats"] for P in Ps], COVERAGE_ADD, ("max_set",))
    kept = W["merge"]["kept"]
    W["coverage_merged"] = {k: per_item(U, [P["coverage_merged"][k] for P in Ps], kept) for k in ("read_length_sum", "path_length")}
    W["coverage_merged"]["stats"] = add_stats(U, [P["coverage_merged"]["stats"] for P in Ps], COVERAGE_ADD, ("max_set",))
    return W


def segments_text(lengths):
    """GFA2 text with one S line per segment (``s<i>``) and no edge: the reads of a graph union, for po_add_gfa."""
    n = len(lengths)
    lines = np.char.add(np.char.add(np.char.add("S\ts", np.arange(n).astype("U")), np.char.add("\t", i64(lengths).astype("U"))), "\t*\n")
    return "H\tVN:z:2.0\n" + "".join(lines.tolist())
