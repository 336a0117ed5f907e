"""The contract of po_layout_diamonds (include/phasm_overlap.h) as plain Python, the composition
of the whole graph-cleaning chain (``removed_by``), and the loader of tests/golden/diamond_cases.npz.

``remove_diamond_tips`` states what the reference's ``remove_diamond_tips`` (phasm/assembly_graph.py:721-743;
phasm/cli/assembler.py:173) computes: sequential, end nodes in node order.  ``remove_diamond_tips_rounds`` is the scheme
the device uses (phasm_amd/csrc/diamond.hip.h): candidates in any order, settled in rounds.  tests/test_diamond_oracle.py
holds both to every golden application, which the reference's own function produced."""
import json
import os
import random

import numpy as np

import reduce_utils as ru
import tips_utils as tu

GOLDEN_FILE = os.path.join(ru.GOLDEN, "diamond_cases.npz")
BRANCHES = ("diamonds", "no_pred1", "no_gt1", "pred1_in_degree_not_1", "pred1_was_gt1", "gt1_lost", "pp_is_gt1",
            "isolated_nodes", "order_sensitive_cases", "asymmetric_second_tips", "chains_with_every_code")
STAGE_FUZZ, STAGE_L, STAGE_B = 1000, 4, 5000     # stage (b): after the reduction and the first tip block at the CLI defaults
STAT_KEYS = ("n_edges_in", "n_edges_out", "n_nodes", "n_nodes_removed", "n_candidates", "n_diamonds", "n_invalid")


def new_counts():
    return {b: 0 for b in BRANCHES}


# ---- the contract, sequential --------------------------------------------------------------------------------------

class _Degrees:
    """Live out-degree per node and the ids of the in-edges (static for a surviving node: only edges INTO a removed node
    ever go)."""

    def __init__(self, edges):
        self.e = [(int(e[0]), int(e[1])) for e in edges]
        assert len(set(self.e)) == len(self.e), "duplicate edge"
        self.out, self.inn = {}, {}
        for k, (u, v) in enumerate(self.e):
            self.out[u] = self.out.get(u, 0) + 1
            self.inn.setdefault(v, []).append(k)

    def candidates(self, order):
        return [n for n in order if self.out.get(n, 0) == 0 and len(self.inn.get(n, ())) == 2]

    def footprint(self, E):
        """The nodes a candidate's decision reads or writes: its two predecessors, and the single predecessor of each
        of them that has in-degree 1."""
        a, b = (self.e[k][0] for k in self.inn[E])
        nodes = [a, b]
        for p in (a, b):
            if len(self.inn.get(p, ())) == 1:
                nodes.append(self.e[self.inn[p][0]][0])
        return nodes

    def decide(self, E):
        """(pred1, gt1) as assembly_graph.py:727-734 leaves them: the LAST predecessor of each shape."""
        pred1 = gt1 = None
        for k in self.inn[E]:
            p = self.e[k][0]
            if self.out[p] == 1 and len(self.inn.get(p, ())) == 1:
                pred1 = p
            if self.out[p] > 1:
                gt1 = p
        return pred1, gt1

    def remove(self, E, pred1, flags):
        """g.remove_node(E); g.remove_node(pred1): the two in-edges of E and the one in-edge of pred1 (whose one
        out-edge is into E).  Returns pp, the predecessor of pred1."""
        k_pp = self.inn[pred1][0]
        pp = self.e[k_pp][0]
        gone = list(self.inn[E]) + [k_pp]
        assert len(set(gone)) == 3 and all(flags[k] == 0 for k in gone), "a diamond removes three distinct live edges"
        for k in self.inn[E]:
            flags[k] = 1
            self.out[self.e[k][0]] -= 1
        flags[k_pp] = 2
        self.out[pp] -= 1
        assert self.out[pred1] == 0
        return pp


def remove_diamond_tips(edges, order, counts=None):
    """edges: (u, v, ...) with distinct (u, v); order: the graph's nodes in node order.  Returns (flags per edge: 0 kept,
    1 in-edge of a removed end node, 2 the in-edge of a removed pred1; the node order left; stats with the names of
    po_diamond_stats)."""
    g = _Degrees(edges)
    order = [int(n) for n in order]
    flags = np.zeros(len(g.e), dtype=np.uint8)
    out0 = dict(g.out)
    removed = set()
    cands = g.candidates(order)
    n_diamonds = 0
    for E in cands:
        assert all(flags[k] == 0 for k in g.inn[E]) and not removed & set(g.footprint(E)[:2]), "in-degrees are static"
        pred1, gt1 = g.decide(E)
        preds = [g.e[k][0] for k in g.inn[E]]
        if pred1 is not None and gt1 is not None:
            pp = g.remove(E, pred1, flags)
            removed.update((E, pred1))
            n_diamonds += 1
            if counts is not None:
                counts["diamonds"] += 1
                counts["pred1_was_gt1"] += out0[pred1] > 1
                counts["pp_is_gt1"] += pp == gt1
        elif counts is not None:
            counts["no_pred1"] += pred1 is None
            counts["no_gt1"] += gt1 is None
            counts["pred1_in_degree_not_1"] += pred1 is None and gt1 is not None and \
                any(g.out[p] == 1 and len(g.inn.get(p, ())) != 1 for p in preds)
            counts["gt1_lost"] += gt1 is None and any(out0[p] > 1 for p in preds)
    left = [n for n in order if n not in removed]
    if counts is not None:
        before, after = set(), set()
        for k, (u, v) in enumerate(g.e):
            before.update((u, v))
            if flags[k] == 0:
                after.update((u, v))
        counts["isolated_nodes"] += len([n for n in left if n in before and n not in after])
    stats = {"n_edges_in": len(g.e), "n_edges_out": int((flags == 0).sum()), "n_nodes": len(order),
             "n_nodes_removed": len(removed), "n_candidates": len(cands), "n_diamonds": n_diamonds, "n_invalid": 0}
    return flags, left, stats


# ---- the contract, in rounds (what the kernels do) -----------------------------------------------------------------

def remove_diamond_tips_rounds(edges, order, seed=0):
    """Flags by the round scheme, and the rounds it took: every unresolved candidate marks its footprint with its rank
    (the lowest wins), a candidate that holds every node of its footprint decides and applies."""
    g = _Degrees(edges)
    order = [int(n) for n in order]
    rank = {n: i for i, n in enumerate(order)}
    flags = np.zeros(len(g.e), dtype=np.uint8)
    unresolved = g.candidates(order)
    random.Random(seed).shuffle(unresolved)                 # the device's candidate list comes in any order
    foot = {E: g.footprint(E) for E in unresolved}          # static: in-degrees never change for a surviving node
    rounds = 0
    while unresolved:
        mark = {}
        for E in unresolved:
            for n in foot[E]:
                mark[n] = min(mark.get(n, rank[E]), rank[E])
        left = []
        for E in unresolved:                                # (resolved candidates of one round share no node)
            if all(mark[n] == rank[E] for n in foot[E]):
                pred1, gt1 = g.decide(E)
                if pred1 is not None and gt1 is not None:
                    g.remove(E, pred1, flags)
            else:
                left.append(E)
        assert len(left) < len(unresolved), "a round resolved nothing"
        unresolved, rounds = left, rounds + 1
    return flags, rounds


# ---- the whole chain, assembler.py:145-182 -------------------------------------------------------------------------

def compose_removed_by(flag_arrays):
    """One byte per stage-1 edge from the flag arrays of reduce, tips, diamonds, tips (each in the order of the edges
    that went into its call): 0 kept; 1 transitive, 2 asymmetric after the reduction; 3 / 4 / 5 incoming tip, outgoing
    tip, asymmetric of the first tip block; 6 / 7 the two diamond flags; 8 / 9 / 10 the second tip block."""
    base = (0, 2, 5, 7)
    out = np.zeros(len(flag_arrays[0]), dtype=np.uint8)
    live = np.arange(len(out))
    for b, f in zip(base, flag_arrays):
        f = np.asarray(f, dtype=np.uint8)
        assert len(f) == len(live)
        out[live[f != 0]] = f[f != 0] + b
        live = live[f == 0]
    return out


def clean_chain(edges, order, fuzz=STAGE_FUZZ, L=STAGE_L, B=STAGE_B, B2=tu.DEFAULT_B, reduce_flags=None):
    """The restatements chained as `phasm layout` chains the reference's functions: (removed_by per input edge, the
    edges left, the node order left, the list of the four stats).  ``reduce_flags``: the flags of the reduction where
    they are known already (ties between equal weights follow the stage-1 insertion order, which ``edges`` must have
    otherwise)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    f0 = np.asarray(reduce_flags, dtype=np.uint8) if reduce_flags is not None else ru.reduce_edges(e, fuzz)
    e1 = e[f0 == 0]
    f1, order1, st1 = tu.remove_tips(e1, order, L, B)
    e2 = e1[f1 == 0]
    f2, order2, st2 = remove_diamond_tips(e2, order1)
    e3 = e2[f2 == 0]
    f3, order3, st3 = tu.remove_tips(e3, order2, L, B2)
    st0 = {"n_edges_in": len(e), "n_transitive": int((f0 == 1).sum()), "n_asymmetric": int((f0 == 2).sum()), "n_edges_out": len(e1)}
    return compose_removed_by([f0, f1, f2, f3]), e3[f3 == 0], order3, [st0, st1, st2, st3]


def chain_counts(stats):
    """The numbers `phasm layout` logs between assembler.py:157 and :182, from the four stats dicts."""
    st0, st1, st2, st3 = stats
    return {"n_transitive": st0["n_transitive"], "n_asymmetric": st0["n_asymmetric"] + st1["n_asymmetric"],
            "n_tip_edges": st1["n_in_tip_edges"] + st1["n_out_tip_edges"], "n_isolated_nodes": st1["n_isolated_nodes"],
            "n_diamonds": st2["n_diamonds"], "n_tip_edges2": st3["n_in_tip_edges"] + st3["n_out_tip_edges"],
            "n_isolated_nodes2": st3["n_isolated_nodes"], "n_asymmetric2": st3["n_asymmetric"]}


# ---- text cases ----------------------------------------------------------------------------------------------------

def union_case(tangle, line):
    """Two seeded read sets side by side in one file, as separate components: ``tangle_case`` of tests/tips_utils.py (tips
    on tips, diamonds, a second tip block with work to do) and ``line_case`` of tests/reduce_utils.py (transitive edges,
    and rows written one way only, which the symmetry pass after the reduction removes) -- a graph in which every step
    of the chain removes something."""
    names, lengths, rows = [], [], []
    for part_names, part_lengths, part_rows in (tu.tangle_case(tangle), ru.line_case(line)):
        off = 2 * len(names)
        names += list(part_names)
        lengths += list(part_lengths)
        rows += [(a + off, b + off, s, e, bs, be) for a, b, s, e, bs, be in part_rows]
    return names, lengths, rows


def case_text(c):
    """GFA2 text of a golden case: the cases of tips_cases.npz by their source, the union cases of this module by seed."""
    if c.get("synth", {}).get("kind") == "union":
        text = ru.gfa_text(*union_case(c["synth"]["tangle"], c["synth"]["line"]))
        assert c.get("text_sha256") in (None, ru.text_digest(text)), "synthetic rows drifted from the golden inputs"
        return text
    return tu.case_text(c)


# ---- golden file ---------------------------------------------------------------------------------------------------

def minus(order, gone):
    gone = set(int(n) for n in gone)
    return [n for n in order if n not in gone]


def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record; beside it per case the arrays that would bloat it.  A node order is kept as
    the nodes that LEFT the order before it (``gone*``): the text cases of tips_cases.npz start from the order that file records, the
    other cases carry theirs (``order``).  Fixed dates, so the same content gives the same bytes."""
    import io
    import zipfile
    arrays, meta = {}, json.loads(json.dumps(obj))
    for i, c in enumerate(meta["cases"]):
        for key in ("order", "edges", "removed_by", "chain_gone"):
            if key in c:
                a = np.asarray(c.pop(key), dtype=np.uint8 if key == "removed_by" else "<i4")
                arrays["c%d.%s" % (i, key)] = a.reshape(-1, 4) if key == "edges" else a
        for j, r in enumerate(c["results"]):
            arrays["c%d.r%d.flags" % (i, j)] = np.frombuffer(bytes.fromhex(r.pop("flags")), dtype=np.uint8)
            for key in ("gone_before", "gone"):
                arrays["c%d.r%d.%s" % (i, j, key)] = np.asarray(r.pop(key), dtype="<i4")
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def load_golden(path=GOLDEN_FILE, tips_golden=None):
    """The record with every node order spelled out: per case ``order`` (stage-1 graph), per result ``order_before``
    and ``order_left``, and for the text cases ``chain["order_left"]`` and ``removed_by``."""
    tips = {c["name"]: c for c in (tips_golden or tu.load_golden())["cases"]}
    with np.load(path) as z:
        obj = json.loads(z["meta"].tobytes().decode())
        for i, c in enumerate(obj["cases"]):
            if "c%d.order" % i in z:
                c["order"] = z["c%d.order" % i].astype(np.int64).tolist()
            else:
                c["order"] = tips[c["name"]]["order"]
            if "c%d.edges" % i in z:
                c["edges"] = z["c%d.edges" % i].astype(np.int64).reshape(-1, 4).tolist()
            if "c%d.removed_by" % i in z:
                c["removed_by"] = z["c%d.removed_by" % i].copy()
                c["chain"]["order_left"] = minus(c["order"], z["c%d.chain_gone" % i].tolist())
            for j, r in enumerate(c["results"]):
                r["flags"] = z["c%d.r%d.flags" % (i, j)].tobytes().hex()
                r["order_before"] = minus(c["order"], z["c%d.r%d.gone_before" % (i, j)].tolist())
                r["order_left"] = minus(r["order_before"], z["c%d.r%d.gone" % (i, j)].tolist())
    return obj
