"""The contract of po_layout_merge (include/phasm_overlap.h) as plain Python, the scheme the
kernels use, the GFA2 lines of the merged graph, two seeded generators and the loader of tests/golden/merge_cases.npz.

``merge_paths`` states what the reference's ``merge_unambiguous_paths`` (phasm/assembly_graph.py:456-541;
phasm/cli/assembler.py:184-186) computes.  ``merge_paths_rounds`` numbers and ranks the way the device does
(phasm_amd/csrc/merge.hip.h): pointer jumping along the links into the nodes, a sort of the heads' ranks.
tests/test_merge_oracle.py holds both to every golden application, which the reference's own function produced."""
import hashlib
import json
import os
import random

import numpy as np

import diamond_utils as du
import reduce_utils as ru
import tips_utils as tu

GOLDEN_FILE = os.path.join(ru.GOLDEN, "merge_cases.npz")
BRANCHES = ("paths", "self_loops", "cycle_nodes", "head_in_degree_gt1", "head_pred_out_gt1", "numbering_differs_from_index_order")
STAT_KEYS = ("n_edges_in", "n_edges_out", "n_nodes", "n_merged", "n_nodes_merged", "max_path_nodes", "n_self_loops",
             "n_cycle_nodes", "n_overflow", "n_invalid")
NONE = -1


def new_counts():
    return {b: 0 for b in BRANCHES}


def _links(e):
    """(out-degree, in-degree, link, back, the edge id of the link out of a node) of distinct edges (u, v, ...)."""
    pairs = [(int(x[0]), int(x[1])) for x in e]
    assert len(set(pairs)) == len(pairs), "duplicate edge"
    out, inn, oute = {}, {}, {}
    for k, (u, v) in enumerate(pairs):
        out[u] = out.get(u, 0) + 1
        inn[v] = inn.get(v, 0) + 1
        oute[u] = k
    link, back = {}, {}
    for k, (u, v) in enumerate(pairs):
        if out[u] == 1 and inn[v] == 1:
            link[u], back[v] = v, u
    return out, inn, link, back, oute


def _result(e, order, lengths, n_nodes, link, back, paths, counts, rounds):
    """Everything the call returns, from the paths in k order (each a list of nodes)."""
    e = np.asarray(e, dtype=np.int64).reshape(-1, 4)
    path_of, offsets, members, prefix, plen, psum = {}, [0], [], [], [], []
    wt = {(int(x[0]), int(x[1])): int(x[2]) for x in e}
    for k, p in enumerate(paths):
        w = [wt[(a, b)] for a, b in zip(p, p[1:])]
        for n in p:
            path_of[n] = k
        members += p
        prefix += w + [0]
        offsets.append(len(members))
        psum.append(sum(w))
        plen.append(sum(w) + int(lengths[p[-1]]))
    flags = np.zeros(len(e), dtype=np.uint8)
    kept, self_loops, overflow = [], 0, 0
    for i, (u, v, w, o) in enumerate(e.tolist()):
        ku, kv = path_of.get(u, NONE), path_of.get(v, NONE)
        if ku != NONE and link.get(u) == v:
            flags[i] = 1
            continue
        if ku != NONE:
            w += psum[ku]
            overflow += not -2**31 <= w < 2**31
            self_loops += ku == kv
            u = n_nodes + ku
        if kv != NONE:
            v = n_nodes + kv
        flags[i] = 2 if (ku != NONE or kv != NONE) else 0
        kept.append((u, v, w, o))
    order_out = [n for n in order if n not in path_of] + [n_nodes + k for k in range(len(paths))]
    cyc = len([n for n in link if n in back and n not in path_of])   # a link in and out, and no head behind them
    stats = {"n_edges_in": len(e), "n_edges_out": len(kept), "n_nodes": len(order), "n_merged": len(paths),
             "n_nodes_merged": len(members), "max_path_nodes": max([len(p) for p in paths] + [0]), "n_self_loops": self_loops,
             "n_cycle_nodes": cyc, "n_overflow": overflow, "n_invalid": 0, "n_rounds": rounds}
    if counts is not None:
        counts["paths"] += len(paths)
        counts["self_loops"] += self_loops
        counts["cycle_nodes"] += cyc
    return {"flags": flags, "edges": np.asarray(kept, dtype=np.int64).reshape(-1, 4), "order": order_out,
            "offsets": np.asarray(offsets, dtype=np.int64), "members": np.asarray(members, dtype=np.int64),
            "prefix": np.asarray(prefix, dtype=np.int64), "lengths": np.asarray(plen, dtype=np.int64), "stats": stats}


def merge_paths(edges, order, lengths, n_nodes=None, counts=None):
    """edges: (u, v, weight, overlap_len) with distinct (u, v); order: the graph's nodes in node order; lengths: length per
    node id; merged node k is written as n_nodes + k (default len(lengths)).  Returns a dict: ``flags`` per edge (0 kept
    as it is, 1 link of a path, 2 kept renamed or re-weighted), ``edges`` kept in input order, ``order`` of the result,
    the tables ``offsets`` / ``members`` / ``prefix`` / ``lengths`` and ``stats`` with the names of po_merge_stats."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    order = [int(n) for n in order]
    n_nodes = len(lengths) if n_nodes is None else n_nodes
    out, inn, link, back, _ = _links(e)
    paths = []
    for n in order:                                  # heads in node order: the numbering
        if n in link and n not in back:
            p = [n]
            while p[-1] in link:                     # (ends: a path never returns to its head, which has no link in)
                p.append(link[p[-1]])
            paths.append(p)
            if counts is not None:
                counts["head_in_degree_gt1"] += inn.get(n, 0) > 1
                counts["head_pred_out_gt1"] += inn.get(n, 0) == 1
    if counts is not None:
        counts["numbering_differs_from_index_order"] += [p[0] for p in paths] != sorted(p[0] for p in paths)
    return _result(e, order, lengths, n_nodes, link, back, paths, counts, None)


def merge_paths_rounds(edges, order, lengths, n_nodes=None, seed=0):
    """The same by the device's scheme: per node (jb, hops, wsum) jumps along ``back`` in rounds, a root pointing at
    itself; a round counts the nodes that reached a root in it and the first that counts none is the last; heads come in
    any order and are sorted by rank."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    order = [int(n) for n in order]
    n_nodes = len(lengths) if n_nodes is None else n_nodes
    rank = {n: 7 * i + 3 for i, n in enumerate(order)}
    out, inn, link, back, oute = _links(e)
    nodes = sorted(set(order) | set(out) | set(inn))
    jb = {n: back.get(n, n) for n in nodes}
    hops = {n: int(n in back) for n in nodes}
    ws = {n: int(e[oute[back[n]], 2]) if n in back else 0 for n in nodes}
    heads = [n for n in nodes if n in link and n not in back]
    random.Random(seed).shuffle(heads)
    max_rounds = 1                                   # ceil(log2(n_nodes)) + 1, the host's cap
    while (1 << (max_rounds - 1)) < len(order):
        max_rounds += 1
    rounds = 0
    while heads and rounds < max_rounds:
        njb = {n: jb[jb[n]] for n in nodes}
        hops = {n: hops[n] + hops[jb[n]] for n in nodes}
        ws = {n: ws[n] + ws[jb[n]] for n in nodes}
        reached = sum(1 for n in nodes if jb[n] in back and njb[n] not in back)
        jb, rounds = njb, rounds + 1
        if not reached:
            break
    heads.sort(key=lambda n: rank[n])
    k_of = {h: k for k, h in enumerate(heads)}
    paths = [[h] for h in heads]
    tail = {}
    for n in nodes:
        if n in back and jb[n] not in back:          # reached its head
            tail.setdefault(jb[n], []).append((hops[n], n, ws[n]))
    for h, rest in tail.items():
        rest.sort()
        assert [x[0] for x in rest] == list(range(1, len(rest) + 1))
        paths[k_of[h]] += [x[1] for x in rest]
    res = _result(e, order, lengths, n_nodes, link, back, paths, None, rounds)
    for k, p in enumerate(paths):                    # the weight sums the jumps carried are the prefix sums
        assert tail[p[0]][-1][2] == int(res["prefix"][res["offsets"][k]:res["offsets"][k + 1]].sum())
    return res


# ---- the file `phasm layout` writes: gfa2_write_graph, phasm/io/gfa.py:281-326 -------------------------------------------

def gfa_lines(res, names, lengths, n_nodes):
    """(H / S / F lines in order, E lines in the result's edge order) of a merged graph.  ``names[n]`` is the name of
    oriented read n with its strand sign.  Stage 1 never emits a weight <= 0, so every prefix but a path's last is
    positive (the reference's writer takes a falsy prefix for the last read)."""
    K = len(res["lengths"])

    def name(n):
        return names[n] if n < n_nodes else "merged%d+" % (n - n_nodes)

    def length(n):
        return int(lengths[n]) if n < n_nodes else int(res["lengths"][n - n_nodes])

    head, seen = ["H\tVN:z:2.0\n"], set()
    for n in res["order"]:
        seg = name(n)[:-1]
        if seg in seen:
            continue
        seen.add(seg)
        head.append("S\t%s\t%d\t*\n" % (seg, length(n)))
        if n >= n_nodes:
            k = n - n_nodes
            assert k < K
            lo, hi = int(res["offsets"][k]), int(res["offsets"][k + 1])
            pre = [int(x) for x in res["prefix"][lo:hi]]
            total, pos = sum(pre), 0
            for read, p in zip(res["members"][lo:hi].tolist(), pre):
                end = pos + p if p else length(n)
                head.append("F\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (seg, name(read), pos, end, p if p else length(n) - total))
                pos += p
    e_lines = ["E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (name(u), name(v), w, length(u), o) for u, v, w, o in res["edges"].tolist()]
    return head, e_lines


def lines_digest(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


# ---- seeded text cases ---------------------------------------------------------------------------------------------

def ring_case(n, seed=None):
    """n reads tiled round a circle: read i ends on read (i + 1) % n.  Each strand is one pure cycle of n links."""
    rng = random.Random(1000 + n if seed is None else seed)
    edges = [(2 * i, 2 * ((i + 1) % n), rng.randrange(400, 1500)) for i in range(n)]
    rng.shuffle(edges)
    return tu._finish(n, tu.edge_rows(edges), "r%d_" % n)


def lasso_case(n, tail=8, seed=None):
    """The ring of ``ring_case`` and a tail of ``tail`` reads that enters it at read 0 (too long for a tip: more than 4
    nodes and more than 5000 bases).  Read 0+ is a head with in-degree 2 and the ring's last read points back at it; on
    the other strand the ring's path ends in read 0-, which has a second out-edge into the tail."""
    assert tail > 4
    rng = random.Random(2000 + 31 * n + tail if seed is None else seed)
    edges = [(2 * i, 2 * ((i + 1) % n), rng.randrange(400, 1500)) for i in range(n)]
    t = [2 * (n + i) for i in range(tail)]
    edges += [(a, b, rng.randrange(1300, 1500)) for a, b in zip(t, t[1:] + [0])]
    rng.shuffle(edges)
    return tu._finish(n + tail, tu.edge_rows(edges), "l%d_%d_" % (n, tail))


SYNTH = {"ring": ring_case, "lasso": lasso_case}


def direct_length(n):
    """The length of node n of a direct case (graphs filled edge by edge have no reads behind them)."""
    return 1000 + int(n) % 97


def case_text(c):
    """GFA2 text of a golden case: the ring and lasso cases of this module, everything else through diamond_utils."""
    kind = c.get("synth", {}).get("kind")
    if kind in SYNTH:
        kw = dict(c["synth"])
        text = ru.gfa_text(*SYNTH[kw.pop("kind")](**kw))
        assert c.get("text_sha256") in (None, ru.text_digest(text)), "synthetic rows drifted from the golden inputs"
        return text
    return du.case_text(c)


# ---- golden file ---------------------------------------------------------------------------------------------------

_RESULT_ARRAYS = (("flags", np.uint8), ("gone_before", "<i4"), ("members", "<i4"), ("prefix", "<i4"), ("path_nodes", "<i4"),
                  ("lengths", "<i8"))


def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record; beside it per result the flags (2 bits per edge, in (u, v) order), the tables
    and the nodes that left the case's node order BEFORE this application (``gone_before``: a node order is kept as a
    difference, as in diamond_cases.npz); per case its order and edges where no other golden file holds them."""
    import io
    import zipfile
    arrays, meta = {}, json.loads(json.dumps(obj))
    for i, c in enumerate(meta["cases"]):
        for key in ("order", "edges", "node_lengths"):
            if key in c:
                a = np.asarray(c.pop(key), dtype="<i4")
                arrays["c%d.%s" % (i, key)] = a.reshape(-1, 4) if key == "edges" else a
        for j, r in enumerate(c["results"]):
            r["flags"] = list(bytes.fromhex(r["flags"]))
            for key, dt in _RESULT_ARRAYS:
                arrays["c%d.r%d.%s" % (i, j, key)] = np.asarray(r.pop(key), dtype=dt)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def load_golden(path=GOLDEN_FILE):
    """The record with every node order spelled out: per case ``order`` (stage-1 graph, or the direct case's own), per
    result ``order_before``, the tables as arrays and ``offsets`` from the path lengths."""
    tips = {c["name"]: c for c in tu.load_golden()["cases"]}
    dia = {c["name"]: c for c in du.load_golden()["cases"]}
    with np.load(path) as z:
        obj = json.loads(z["meta"].tobytes().decode())
        for i, c in enumerate(obj["cases"]):
            if "c%d.order" % i in z:
                c["order"] = z["c%d.order" % i].astype(np.int64).tolist()
            else:
                c["order"] = (tips.get(c["name"]) or dia[c["name"]])["order"]
            if "c%d.edges" % i in z:
                c["edges"] = z["c%d.edges" % i].astype(np.int64).reshape(-1, 4).tolist()
            if "c%d.node_lengths" % i in z:
                c["node_lengths"] = z["c%d.node_lengths" % i].astype(np.int64).tolist()
            for j, r in enumerate(c["results"]):
                for key, _ in _RESULT_ARRAYS:
                    r[key] = z["c%d.r%d.%s" % (i, j, key)].astype(np.int64)
                r["flags"] = r["flags"].astype(np.uint8).tobytes().hex()
                r["order_before"] = du.minus(c["order"], r.pop("gone_before").tolist())
                r["offsets"] = np.concatenate([[0], np.cumsum(r.pop("path_nodes"))]).astype(np.int64)
    return obj


def check_against_record(res, rec, e_sorted_input):
    """``res`` (a ``merge_paths`` dict computed on the input edges in (u, v) order) against one golden record."""
    assert np.array_equal(res["flags"], ru.unpack_flags(rec["flags"], len(e_sorted_input)))
    for key in ("offsets", "members", "prefix", "lengths"):
        assert np.array_equal(res[key], rec[key]), key
    assert ru.edge_digest(ru.sort_edges(res["edges"])) == rec["kept_sha256"]
    assert res["order"] == du.minus(rec["order_before"], rec["members"].tolist()) + \
        [rec["n_ids"] + k for k in range(len(rec["lengths"]))]
    st = res["stats"]
    assert {k: st[k] for k in STAT_KEYS} == {k: rec[k] for k in STAT_KEYS}
