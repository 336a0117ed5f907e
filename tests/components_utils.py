"""The contract of po_layout_components (include/phasm_overlap.h) as plain Python, the scheme the
kernels use run synchronously, the direct cases, the file lines of the component writers and the loader of
tests/golden/components_cases.npz.

``weak_components`` states what ``networkx.weakly_connected_components`` yields on a graph with the given node insertion
order (phasm/cli/assembler.py:289-304): component i is the i-th in the order of each component's lowest-ranked node.
``components_rounds`` reaches the same partition the way the device does (phasm_amd/csrc/components.hip.h): one parent
word per rank, hooking over the edges and pointer jumping, in rounds, until a round lowers no word."""
import hashlib
import json
import os
import random

import numpy as np

import reduce_utils as ru

GOLDEN_FILE = os.path.join(ru.GOLDEN, "components_cases.npz")
DIGEST_ABOVE = 3000      # applications with more edges keep digests of their arrays
STAT_KEYS = ("n_nodes", "n_edges", "n_components", "n_singletons", "max_component_nodes", "max_component_edges")


def _result(order, uv, root_of_rank):
    """Everything the call returns, from the root rank of every rank."""
    n = len(order)
    roots = sorted(set(root_of_rank))
    number = {r: i for i, r in enumerate(roots)}
    node_comp = np.asarray([number[r] for r in root_of_rank], dtype=np.int64)
    rank = {x: i for i, x in enumerate(order)}
    edge_comp = np.asarray([node_comp[rank[u]] for u, _ in uv], dtype=np.int64)
    n_nodes = np.bincount(node_comp, minlength=len(roots)).astype(np.int64) if n else np.zeros(0, np.int64)
    n_edges = np.bincount(edge_comp, minlength=len(roots)).astype(np.int64) if len(roots) else np.zeros(0, np.int64)
    first = np.asarray([order[r] for r in roots], dtype=np.int64)
    stats = {"n_nodes": n, "n_edges": len(uv), "n_components": len(roots), "n_singletons": int((n_nodes == 1).sum()),
             "max_component_nodes": int(n_nodes.max()) if len(roots) else 0,
             "max_component_edges": int(n_edges.max()) if len(roots) else 0}
    return {"node_component": node_comp, "edge_component": edge_comp, "first_node": first, "n_nodes": n_nodes, "n_edges": n_edges,
            "stats": stats}


def uv_of(edges):
    """The (u, v) columns of an edge list of any width as an int64 array [n, 2]."""
    if len(edges) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.asarray(edges, dtype=np.int64).reshape(len(edges), -1)[:, :2]


def _pairs(edges):
    return [(int(x[0]), int(x[1])) for x in edges]


def weak_components(edges, order):
    """edges: rows that start with (u, v); order: the graph's nodes in node order.  A plain union-find whose roots are the
    lowest rank of their set.  Returns ``node_component`` (parallel to ``order``), ``edge_component`` (the component of u,
    input order), per component ``first_node`` / ``n_nodes`` / ``n_edges`` and ``stats`` with the names of
    po_components_stats.  An edge end outside the order raises ValueError."""
    order = [int(x) for x in order]
    rank = {x: i for i, x in enumerate(order)}
    assert len(rank) == len(order), "a node twice in the order"
    uv = _pairs(edges)
    parent = list(range(len(order)))

    def find(r):
        while parent[r] != r:
            parent[r] = parent[parent[r]]
            r = parent[r]
        return r

    for u, v in uv:
        if u not in rank or v not in rank:
            raise ValueError("an edge has an end that is not in the node order")
        a, b = find(rank[u]), find(rank[v])
        if a != b:
            parent[max(a, b)] = min(a, b)
    return _result(order, uv, [find(r) for r in range(len(order))])


def components_rounds(edges, order):
    """The same by the device's scheme, every kernel of a round reading the words as the kernel before left them: hook
    (per edge, the lower of the two parents into the higher parent and into both ends), then jump (p[r] = p[p[r]]).  The
    first round that lowers no word is the last; it is counted.  ``stats["rounds"]`` is that count."""
    order = [int(x) for x in order]
    rank = {x: i for i, x in enumerate(order)}
    uv = _pairs(edges)
    n = len(order)
    ru_ = np.asarray([rank[u] for u, _ in uv], dtype=np.int64)
    rv_ = np.asarray([rank[v] for _, v in uv], dtype=np.int64)
    p = np.arange(n, dtype=np.int64)
    rounds, cap = 0, n + 2
    while n and rounds < cap:
        before = p.copy()
        pu, pv = before[ru_], before[rv_]
        lo, hi = np.minimum(pu, pv), np.maximum(pu, pv)
        for target in (hi, ru_, rv_):
            np.minimum.at(p, target, lo)
        hooked = p.copy()
        p = np.minimum(hooked, hooked[hooked])
        rounds += 1
        if np.array_equal(p, before):
            break
    else:
        assert n == 0, "the rounds reached their cap"
    assert (p[p] == p).all() and (p <= np.arange(n)).all() and (p[ru_] == p[rv_]).all()
    res = _result(order, uv, p.tolist())
    res["stats"]["rounds"] = rounds
    return res


# ---- direct cases: edges (u, v) plus an explicit node order ---------------------------------------------------------------

def _path(nodes):
    return list(zip(nodes, nodes[1:]))


def direct_inputs():
    """(name, order, edges, n_ids or None).  Nodes are even ids unless a case is about the other strand; ``n_ids`` is given
    where ids at or above it name merged nodes."""
    ev = lambda n, at=0: [at + 2 * i for i in range(n)]   # noqa: E731
    cases = [("empty", [], [], None), ("nodes_without_edges", [4, 2, 0], [], None), ("one_edge", [0, 2], [(0, 2)], None),
             ("one_self_loop", [0, 2], [(2, 2)], None), ("two_cycle", [2, 0], [(0, 2), (2, 0)], None)]
    for leaves in (64, 65):
        lv, centre = ev(leaves), 2 * leaves
        cases.append(("star_%d_centre_last" % leaves, lv + [centre],
                      [(centre, x) if i % 3 else (x, centre) for i, x in enumerate(lv)], None))
    for n in (2, 64, 65, 257, 1025):
        cases.append(("path_%d" % n, ev(n), _path(ev(n)), None))
    ids = ev(4097)
    scr = list(ids)
    random.Random(4097).shuffle(scr)
    zig = [ids[i // 2] if i % 2 == 0 else ids[-1 - i // 2] for i in range(len(ids))]
    for tag, order in (("identity", ids), ("reversed", ids[::-1]), ("scrambled", scr), ("zigzag", zig)):
        cases.append(("path_4097_" + tag, order, _path(ids), None))
    for K in (1025, 2050):   # (2 050 pairs: 4 100 ranks, roots on both sides of the prefix sum's first 4 096)
        order = [x for i in reversed(range(K)) for x in (4 * i, 4 * i + 2)]
        cases.append(("pairs_%d_heads_against_ids" % K, order, [(4 * i, 4 * i + 2) for i in range(K)], None))
    cases.append(("path_and_its_mirror_interleaved", [0, 7, 2, 5, 4, 3, 6, 1], _path([0, 2, 4, 6]) + _path([7, 5, 3, 1]), None))
    cases.append(("lowest_rank_reached_against_the_edges", [0, 2, 4, 6], [(2, 0), (4, 2), (4, 6)], None))
    cases.append(("merged_ids", [9, 0, 8, 3, 10, 6], [(8, 0), (3, 9), (10, 10), (9, 8)], 8))
    return cases


# ---- what the component writers write (phasm/io/gfa.py:250-326 on g.subgraph(component)) -------------------------------

def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype="<i8")).tobytes())
    return h.hexdigest()


def lines_digest(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def block_digest(blocks):
    """Digest of a set of line blocks (an S line with its F lines), order ignored: a subgraph's node order is a set's."""
    return lines_digest(sorted("".join(b) for b in blocks))


def split_blocks(lines):
    """(blocks, other lines) of a written component: a block is an ``S`` line with the ``F`` lines behind it; the header
    is dropped, the ``E`` / ``L`` lines are the other lines."""
    blocks, rest = [], []
    for ln in lines:
        if ln[0] == "S":
            blocks.append([ln])
        elif ln[0] == "F":
            blocks[-1].append(ln)
        elif ln[0] != "H":
            rest.append(ln)
    return blocks, rest


def writers_digest(per_component):
    """One digest of what the two writers write for every component, in component order: ``per_component`` yields
    (GFA2 lines, GFA1 lines).  Blocks count as a set, ``E`` and ``L`` lines sorted; both files must start with their header."""
    parts = []
    for gfa2, gfa1 in per_component:
        assert gfa2[0] == "H\tVN:z:2.0\n" and gfa1[0] == "H\tVN:z:1.0\n"
        for lines in (gfa2, gfa1):
            blocks, rest = split_blocks(lines)
            parts += [block_digest(blocks), lines_digest(sorted(rest))]
    return lines_digest(parts)


def graph_file_record(graph, comps):
    """The golden record of a graph file's reconstruction: ``graph`` with ``node_order`` and ``edges`` (phasm_amd.io.gfa
    GraphFile numbering), ``comps`` a ``weak_components`` result on it."""
    e = np.asarray(graph.edges, dtype=np.int64).reshape(-1, 4)
    return dict(record_of(comps), file_order=[int(n) for n in graph.node_order], file_edges_sha256=digest(e[np.lexsort((e[:, 1], e[:, 0]))]))


# hand-written graph files, each aimed at one rule of the reader (tests/golden/make_components_golden.py runs the
# reference's two functions on them)
HAND_FILES = {
    "dollar_positions": "H\tVN:z:2.0\nS\ta\t100\t*\nS\tb\t90\t*\nE\t*\ta+\tb+\t40\t100$\t0\t60\t*\nE\t*\tb-\ta-\t30$\t90$\t0$\t55\t*\n",
    "duplicated_edge_line": "S\ta\t100\t*\nS\tb\t90\t*\nS\tc\t80\t*\nE\t*\ta+\tb+\t40\t100\t0\t60\t*\nE\t*\tb+\tc+\t50\t90\t0\t40\t*\n"
                            "E\t*\ta+\tb+\t45\t100\t5\t70\t*\n",
    "segments_without_edges_between": "S\tlone0\t10\t*\nS\ta\t100\t*\nS\tlone1\t11\t*\nS\tb\t90\t*\nS\tlone2\t12\t*\n"
                                      "E\t*\tb+\ta+\t40\t90\t0\t50\t*\n",
    "minus_strand_only": "S\ta\t100\t*\nS\tb\t90\t*\nS\tc\t70\t*\nE\t*\tb-\ta-\t40\t90\t0\t50\t*\n",
    "merged_segment_without_edges": "S\ta\t100\t*\nS\tmerged0\t150\t*\nF\tmerged0\tx+\t0\t60\t0\t60\t*\nF\tmerged0\ty-\t60\t150\t0\t90\t*\n"
                                    "S\tb\t90\t*\nE\t*\ta+\tb+\t40\t100\t0\t60\t*\n",
    "merged_segment_fragments_out_of_order": "S\tmerged0\t150\t*\nF\tmerged0\ty-\t60\t150\t0\t90\t*\nF\tmerged0\tx+\t0\t60\t0\t60\t*\n"
                                             "S\ta\t100\t*\nS\ta\t101\t*\nE\t*\tmerged0+\ta-\t120\t150\t0\t30\t*\nE\t*\ta+\tmerged0+\t80\t101\t0\t25\t*\n",
}


# ---- golden file ---------------------------------------------------------------------------------------------------

def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record; every list of integers of a record that is longer than 8 goes beside it as an
    array named by its place in the record."""
    import io
    import zipfile
    arrays = {}

    def walk(o, where):
        if isinstance(o, dict):
            return {k: walk(v, where + "." + k) for k, v in o.items()}
        if isinstance(o, np.ndarray) or (isinstance(o, list) and len(o) > 8 and all(isinstance(x, (int, np.integer)) for x in o)):
            arrays[where] = np.asarray(o, dtype="<i8")
            lo, hi = (int(arrays[where].min()), int(arrays[where].max())) if arrays[where].size else (0, 0)
            if -2**31 <= lo and hi < 2**31:
                arrays[where] = arrays[where].astype("<i4")
            return {"__array__": where}
        if isinstance(o, list):
            return [walk(v, "%s.%d" % (where, i)) for i, v in enumerate(o)]
        return o

    meta = walk(json.loads(json.dumps(obj, default=lambda a: a.tolist())), "r")
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


_GOLDEN = []


def load_golden(path=GOLDEN_FILE):
    if path == GOLDEN_FILE and _GOLDEN:
        return _GOLDEN[0]
    with np.load(path) as z:
        def walk(o):
            if isinstance(o, dict):
                if set(o) == {"__array__"}:
                    return z[o["__array__"]].astype(np.int64).tolist()
                return {k: walk(v) for k, v in o.items()}
            if isinstance(o, list):
                return [walk(v) for v in o]
            return o
        obj = walk(json.loads(z["meta"].tobytes().decode()))
    if path == GOLDEN_FILE:
        _GOLDEN.append(obj)
    return obj


def record_of(res, rounds=None):
    """The golden record of one application from a ``weak_components`` result: arrays, or their digests above DIGEST_ABOVE edges."""
    rec = dict(res["stats"])
    rec.pop("rounds", None)
    if rounds is not None:
        rec["rounds"] = rounds
    keys = ("node_component", "first_node", "n_nodes", "n_edges")
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = digest(*[res[k] for k in keys])
    else:
        for k in keys:
            rec["c_" + k if k.startswith("n_") else k] = np.asarray(res[k]).tolist()
    return rec


def check_against_record(res, rec):
    """A ``weak_components``-shaped result (of any producer) against one golden record."""
    assert {k: res["stats"][k] for k in STAT_KEYS} == {k: rec[k] for k in STAT_KEYS}
    keys = ("node_component", "first_node", "n_nodes", "n_edges")
    if "sha256" in rec:
        assert digest(*[res[k] for k in keys]) == rec["sha256"]
    else:
        for k in keys:
            assert np.asarray(res[k]).tolist() == rec["c_" + k if k.startswith("n_") else k], k
    assert len(res["edge_component"]) == rec["n_edges"]
