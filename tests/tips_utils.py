"""The contract of po_layout_tips and po_result_node_order (include/phasm_overlap.h) as plain
Python, the seeded synthetic cases of tests/golden/tips_cases.npz, and the loader of that file.

``remove_tips`` states what the reference's ``remove_incoming_tips`` + ``remove_outgoing_tips`` + ``make_symmetric`` +
``clean_graph`` (phasm/assembly_graph.py:267-394, :429-453; phasm/cli/assembler.py:161-167) compute: sequential, tips in
node order.  ``remove_tips_rounds`` is the scheme the device uses (phasm_amd/csrc/tips.hip.h): candidates in any order,
settled in rounds.  ``node_order`` is the rule by which po_layout_edges derives the reference's graph order from the
rows.  tests/test_tips_oracle.py holds all three to every golden case, which the reference's own functions produced."""
import json
import os
import random

import numpy as np

import reduce_utils as ru
from oracle import layout_oracle as lo

GOLDEN_FILE = os.path.join(ru.GOLDEN, "tips_cases.npz")
BRANCHES = ("end_length", "end_bases", "end_junction", "end_dead_end", "through_emptied_junction", "order_sensitive_cases",
            "asymmetric_after_tips", "isolated_nodes", "weight_le0_walked")
DEFAULT_L, DEFAULT_B = 4, 5000


def new_counts():
    return {b: 0 for b in BRANCHES}


# ---- the node order ------------------------------------------------------------------------------------------------

def node_order(rows, lengths, min_read_length=0, min_overlap_length=0, max_overhang_abs=1000, max_overhang_rel=0.8, with_rows=False):
    """Oriented nodes in the order the reference's graph first saw them, without the nodes of contained reads.
    rows: (a, b, astart, aend, bstart, bend) in file order; lengths per oriented node.  ``with_rows``: the pair (that
    order, the index of the row that brought each node in)."""
    rows = [tuple(int(x) for x in r) for r in rows]
    first_c, types, passes = {}, [], []
    for r, (a, b, s, e, bs, be) in enumerate(rows):
        la, lb = int(lengths[a]), int(lengths[b])
        t = lo.classify(s, e, bs, be, la, lb)
        types.append(t)
        ok = t in (lo.OVERLAP_AB, lo.OVERLAP_BA)
        if t == lo.A_CONTAINED:
            first_c.setdefault(a, r)
        elif t == lo.B_CONTAINED:
            first_c.setdefault(b, r)
        else:
            ovl = lo.overlap_length(s, e, bs, be)
            if min_read_length and (la < min_read_length or lb < min_read_length):
                ok = False
            elif min_overlap_length and ovl < min_overlap_length:
                ok = False
            elif not lo.overhang(s, e, bs, be, la, lb) <= min(max_overhang_abs, max_overhang_rel * ovl):
                ok = False
        passes.append(ok)
    contained_reads = {n >> 1 for n in first_c}
    rank = {}
    for r, (a, b, *_rest) in enumerate(rows):
        if not passes[r] or first_c.get(a, len(rows)) <= r or first_c.get(b, len(rows)) <= r:
            continue
        slots = (a, b, b ^ 1, a ^ 1) if types[r] == lo.OVERLAP_AB else (b, a, a ^ 1, b ^ 1)
        for s, n in enumerate(slots):
            if (n >> 1) not in contained_reads:
                rank.setdefault(n, (r, s))
    order = sorted(rank, key=rank.get)
    return (order, [rank[n][0] for n in order]) if with_rows else order


# ---- the contract, sequential --------------------------------------------------------------------------------------

class _Graph:
    def __init__(self, edges):
        self.e = [(int(e[0]), int(e[1]), int(e[2])) for e in edges]
        self.out, self.inn = {}, {}
        for k, (u, v, _) in enumerate(self.e):
            self.out.setdefault(u, set()).add(k)
            self.inn.setdefault(v, set()).add(k)
        assert len({(u, v) for u, v, _ in self.e}) == len(self.e), "duplicate edge"

    def side(self, rev):
        """(forward edge sets, backward edge sets, index of an edge's far end) for a walk with or against the edges."""
        return (self.inn, self.out, 0) if rev else (self.out, self.inn, 1)

    def remove(self, k):
        u, v, _ = self.e[k]
        self.out[u].discard(k)
        self.inn[v].discard(k)


def _walk(g, s, rev, L, B, counts=None, deg0=None):
    """The loop of remove_incoming_tips (assembly_graph.py:355-372) from tip s: (is_tip, edge ids of the path)."""
    fwd, bwd, far = g.side(rev)
    path, curr, total = [], s, 0
    while len(fwd.get(curr, ())) == 1 and len(bwd.get(curr, ())) <= 1:
        if counts is not None and curr != s and deg0[curr] > 1:
            counts["through_emptied_junction"] += 1
        k = next(iter(fwd[curr]))
        path.append(k)
        curr = g.e[k][far]
        total += g.e[k][2]
        if counts is not None:
            counts["weight_le0_walked"] += g.e[k][2] <= 0
        if len(path) + 1 > L + 1:
            if counts is not None:
                counts["end_length"] += 1
            return False, path
        if total > B:
            if counts is not None:
                counts["end_bases"] += 1
            return False, path
    if counts is not None:
        # (a node with several out-edges ends a walk like one with several in-edges: both count as junctions)
        counts["end_dead_end" if len(bwd.get(curr, ())) <= 1 and not fwd.get(curr) else "end_junction"] += 1
    return True, path


def _tips_pass(g, order, rev, L, B, flags, which, counts=None):
    fwd, bwd, _ = g.side(rev)
    deg0 = {n: len(bwd.get(n, ())) for n in order}
    tips = [n for n in order if not bwd.get(n)]
    n_cand = 0
    for s in tips:
        if len(fwd.get(s, ())) != 1:
            continue
        n_cand += 1
        is_tip, path = _walk(g, s, rev, L, B, counts, deg0)
        if is_tip:
            for k in path:
                g.remove(k)
                flags[k] = which
    return n_cand


def remove_tips(edges, order, L=DEFAULT_L, B=DEFAULT_B, counts=None):
    """edges: (u, v, weight[, ...]) with distinct (u, v); order: the graph's nodes in node order.  Returns (flags per
    edge: 0 kept, 1 incoming-tip edge, 2 outgoing-tip edge, 3 removed by the symmetry pass; the node order left;
    stats with the names of po_tips_stats)."""
    g = _Graph(edges)
    order = [int(n) for n in order]
    flags = np.zeros(len(g.e), dtype=np.uint8)
    c_in = _tips_pass(g, order, 0, L, B, flags, 1, counts)
    c_out = _tips_pass(g, order, 1, L, B, flags, 2, counts)
    index = {(u, v): k for k, (u, v, _) in enumerate(g.e)}
    live = flags == 0
    for (u, v), k in index.items():
        if live[k]:
            t = index.get((v ^ 1, u ^ 1))
            if t is None or not live[t]:
                flags[k] = 3
    alive = set()
    for k, (u, v, _) in enumerate(g.e):
        if flags[k] == 0:
            alive.update((u, v))
    left = [n for n in order if n in alive]
    stats = {"n_edges_in": len(g.e), "n_in_tip_edges": int((flags == 1).sum()), "n_out_tip_edges": int((flags == 2).sum()),
             "n_asymmetric": int((flags == 3).sum()), "n_edges_out": int((flags == 0).sum()), "n_nodes": len(order),
             "n_isolated_nodes": len(order) - len(left), "n_candidates_in": c_in, "n_candidates_out": c_out}
    if counts is not None:
        counts["asymmetric_after_tips"] += stats["n_asymmetric"]
        counts["isolated_nodes"] += stats["n_isolated_nodes"]
    return flags, left, stats


# ---- the contract, in rounds (what the kernels do) -----------------------------------------------------------------

def _rounds_pass(g, order, rev, L, B, flags, which, rng):
    fwd, bwd, far = g.side(rev)
    rank = {n: i for i, n in enumerate(order)}
    cand = [n for n in order if not bwd.get(n) and len(fwd.get(n, ())) == 1]
    rng.shuffle(cand)                                   # the device's candidate list comes in any order
    unresolved, rounds = cand, 0
    while unresolved:
        mark = {}
        for s in unresolved:                            # k_tips_mark: the chain, whatever the in-degrees
            curr, n = s, 1
            mark[curr] = min(mark.get(curr, rank[s]), rank[s])
            while n < L + 2 and len(fwd.get(curr, ())) == 1:
                curr = g.e[next(iter(fwd[curr]))][far]
                n += 1
                mark[curr] = min(mark.get(curr, rank[s]), rank[s])
        left, apply = [], []
        for s in unresolved:                            # k_tips_resolve, decisions on the graph as the round found it
            is_tip, path = _walk(g, s, rev, L, B)
            nodes = [s] + [g.e[k][far] for k in path]
            if all(mark[n] == rank[s] for n in nodes):
                if is_tip:
                    apply.append(path)
            else:
                left.append(s)
        for path in apply:
            for k in path:
                g.remove(k)
                flags[k] = which
        assert len(left) < len(unresolved), "a round resolved nothing"
        unresolved, rounds = left, rounds + 1
    return rounds


def remove_tips_rounds(edges, order, L=DEFAULT_L, B=DEFAULT_B, seed=0):
    """Flags of the two tip passes only (0, 1, 2) by the round scheme, and the rounds each pass took."""
    g = _Graph(edges)
    order = [int(n) for n in order]
    flags = np.zeros(len(g.e), dtype=np.uint8)
    rng = random.Random(seed)
    r_in = _rounds_pass(g, order, 0, L, B, flags, 1, rng)
    r_out = _rounds_pass(g, order, 1, L, B, flags, 2, rng)
    return flags, r_in, r_out


# ---- seeded synthetic cases ----------------------------------------------------------------------------------------

READ_LEN = 20000


def edge_rows(edges):
    """One row per (u, v, weight) between reads of READ_LEN bases, built like ``hub_case`` in reduce_utils: astart =
    weight, bstart = 0, the alignment ends at a's end -- the edge (u, v) and its mirror twin (v^1, u^1), both of that
    weight (0 < weight < READ_LEN)."""
    return [(u, v, w, READ_LEN, 0, READ_LEN - w) for u, v, w in edges]


def _finish(n_reads, rows, prefix):
    return ["%s%d" % (prefix, i) for i in range(n_reads)], [READ_LEN] * n_reads, rows


JUNCTION_ORDERS = ("a_first", "b_first", "a_last_edge_first", "spine_first", "b_then_spine")


def junction_case(order="a_first"):
    """Two incoming chains on one junction J that heads a chain of 8: a0 -> a1 -> J and b0 -> J.  Which chain the
    reference visits first decides what goes: A first removes (a0, a1), (a1, J) and leaves b0 -> J (J's in-degree is 1
    by then, and the walk from b0 runs into the length bound); B first removes (b0, J) only."""
    a0, a1, b0, J = 0, 2, 4, 6
    spine = [(J + 2 * i, J + 2 * i + 2, 900) for i in range(8)]
    A, B = [(a0, a1, 700), (a1, J, 800)], [(b0, J, 600)]
    edges = {"a_first": A + B + spine, "b_first": B + A + spine, "a_last_edge_first": [A[1], B[0], A[0]] + spine,
             "spine_first": spine + A + B, "b_then_spine": B + spine + A}[order]
    return _finish(12, edge_rows(edges), "j")


def comb_case(L=4, B=DEFAULT_B):
    """A line of 60 reads with teeth: incoming and outgoing tips of 1 to L + 2 edges, and tips of two edges and of one
    edge whose base sums are B - 1, B and B + 1 (the one-edge teeth meet the base bound at L = 1 too, where a tooth of
    two edges ends at the length bound first)."""
    n = 0

    def fresh():
        nonlocal n
        n += 1
        return 2 * (n - 1)

    line = [fresh() for _ in range(60)]
    edges = [(line[i], line[i + 1], 1000) for i in range(59)]
    at = 3
    for k in range(1, L + 3):
        for incoming in (True, False):
            chain = [fresh() for _ in range(k)]
            if incoming:
                nodes = chain + [line[at]]
            else:
                nodes = [line[at]] + chain
            edges += [(nodes[i], nodes[i + 1], 300) for i in range(k)]
            at += 2
    for total in (B - 1, B, B + 1):
        for incoming in (True, False):
            x, y = fresh(), fresh()
            nodes = [x, y, line[at]] if incoming else [line[at], x, y]
            edges += [(nodes[0], nodes[1], total - 2000), (nodes[1], nodes[2], 2000)]
            at += 2
            x = fresh()
            edges.append((x, line[at], total) if incoming else (line[at], x, total))
            at += 1
    assert at < 58
    random.Random(L).shuffle(edges)
    return _finish(n, edge_rows(edges), "c")


def tangle_case(seed, n_line=30, n_tips=26, L=4):
    """A line, tips of random length and weight hung on it and ON EACH OTHER's ends on random strands (a junction emptied
    by earlier tips lets a later walk through into the next junction: cascades), two small components shorter than the
    bound, and reads that bring a node into the graph through a row to a read that a LATER row finds contained."""
    rng = random.Random(seed)
    n = 0

    def fresh():
        nonlocal n
        n += 1
        return 2 * (n - 1) + (rng.random() < 0.3)

    line = [fresh() for _ in range(n_line)]
    edges = [(line[i], line[i + 1], rng.randrange(400, 1500)) for i in range(n_line - 1)]
    targets = line[2:-2]
    for _ in range(n_tips):
        k = rng.randrange(1, L + 3)
        chain = [fresh() for _ in range(k)]
        w = [rng.choice([200, 900, 1300, 2499, 2500, 2501, 4999]) for _ in range(k)]
        j = rng.choice(targets)
        if rng.random() < 0.5:
            nodes = chain + [j]
        else:
            nodes = [j] + chain
        edges += [(nodes[i], nodes[i + 1], w[i]) for i in range(k)]
        if rng.random() < 0.6:
            targets.append(rng.choice(chain))           # later tips may end on this one
    for _ in range(2):                                  # whole components shorter than the bound
        comp = [fresh() for _ in range(rng.randrange(2, 4))]
        edges += [(comp[i], comp[i + 1], 500) for i in range(len(comp) - 1)]
    seen, uniq = set(), []
    for u, v, w in edges:
        if (u, v) not in seen and (v ^ 1, u ^ 1) not in seen and u >> 1 != v >> 1:
            seen.add((u, v))
            uniq.append((u, v, w))
    rng.shuffle(uniq)
    rows = edge_rows(uniq)
    # x -> y early, "y is contained in z" at the very end: x (and x^1) are in the graph, y never is
    late = []
    for _ in range(3):
        x, y, z = fresh() & ~1, fresh() & ~1, fresh() & ~1
        at = rng.randrange(len(rows) // 2)
        rows.insert(at, (x, y, 700, READ_LEN, 0, READ_LEN - 700))
        if rng.random() < 0.5:
            rows.insert(at + 1, (rng.choice(line), x, 650, READ_LEN, 0, READ_LEN - 650))
        late.append((y, z, 0, READ_LEN, 0, READ_LEN))
    return _finish(n, rows + late, "t%d_" % seed)


def selfish_case(seed, n_line=24):
    """What stage 1 emits for a read aligned with itself and with its own reverse strand, with tips around it: a row
    (x, x) gives the self-loops (x, x) and (x^1, x^1); a row (x, x^1) gives the one edge (x, x^1), which is its own
    twin; rows (x, y) and (y, x) give a 2-cycle.  Such reads sit on a line and at the ends of tips, and tips of one to
    three edges run into them, several into the same one."""
    rng = random.Random(seed)
    n = 0

    def fresh():
        nonlocal n
        n += 1
        return 2 * (n - 1) + (rng.random() < 0.3)

    line = [fresh() for _ in range(n_line)]
    edges = [(line[i], line[i + 1], rng.randrange(400, 1500)) for i in range(n_line - 1)]
    special = []
    for kind in ("loop", "flip", "cycle") * 4:
        x = fresh()
        if kind == "loop":
            edges.append((x, x, rng.randrange(50, 900)))
        elif kind == "flip":
            edges.append((x, x ^ 1, rng.randrange(50, 900)))
        else:
            y = fresh()
            edges += [(x, y, rng.randrange(50, 900)), (y, x, rng.randrange(50, 900))]
        if rng.random() < 0.5:                          # on the line, or left to the tips alone
            j = rng.choice(line[2:-2])
            edges.append((j, x, 800) if rng.random() < 0.5 else (x, j, 800))
        special.append(x)
    for _ in range(20):
        k = rng.randrange(1, 4)
        chain = [fresh() for _ in range(k)]
        j = rng.choice(special + special + line[2:-2])
        nodes = chain + [j] if rng.random() < 0.6 else [j] + chain
        edges += [(nodes[i], nodes[i + 1], rng.choice([300, 1200, 2500, 4999])) for i in range(k)]
    seen, uniq = set(), []
    for u, v, w in edges:
        if (u, v) not in seen and (v ^ 1, u ^ 1) not in seen:
            seen.add((u, v))
            uniq.append((u, v, w))
    rng.shuffle(uniq)
    return _finish(n, edge_rows(uniq), "s%d_" % seed)


SYNTH = {"junction": junction_case, "comb": comb_case, "tangle": tangle_case, "selfish": selfish_case}


def case_text(c):
    """GFA2 text of a golden case (the reduce goldens' cases by their name, the synthetic ones of this module by seed)."""
    if "reduce_case" in c:
        return ru.case_text(next(x for x in ru.load_golden()["cases"] if x["name"] == c["reduce_case"]))
    kw = dict(c["synth"])
    text = ru.gfa_text(*SYNTH[kw.pop("kind")](**kw))
    assert c.get("text_sha256") in (None, ru.text_digest(text)), "synthetic rows drifted from the golden inputs"
    return text


# ---- golden file ---------------------------------------------------------------------------------------------------

def by_uv(arr):
    arr = np.asarray(arr, dtype=np.int64).reshape(-1, 4)
    return np.lexsort((arr[:, 1], arr[:, 0])) if len(arr) else np.empty(0, dtype=np.int64)


def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record; node orders, direct edge lists and flags (2 bits per edge, in (u, v) order)
    as arrays beside it.  Fixed dates, so the same content gives the same bytes."""
    import io
    import zipfile
    arrays, meta = {}, json.loads(json.dumps(obj))
    for i, c in enumerate(meta["cases"]):
        arrays["c%d.order" % i] = np.asarray(c.pop("order"), dtype="<i4")
        if "edges" in c:
            arrays["c%d.edges" % i] = np.asarray(c.pop("edges"), dtype="<i4").reshape(-1, 4)
        for j, r in enumerate(c["results"]):
            for key in ("flags", "flags2"):
                if key in r:
                    arrays["c%d.r%d.%s" % (i, j, key)] = np.frombuffer(bytes.fromhex(r.pop(key)), dtype=np.uint8)
            for key in ("order_left", "order_left2"):
                if key in r:
                    arrays["c%d.r%d.%s" % (i, j, key)] = np.asarray(r.pop(key), dtype="<i4")
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def load_golden(path=GOLDEN_FILE):
    with np.load(path) as z:
        obj = json.loads(z["meta"].tobytes().decode())
        for i, c in enumerate(obj["cases"]):
            c["order"] = z["c%d.order" % i].astype(np.int64).tolist()
            if "c%d.edges" % i in z:
                c["edges"] = z["c%d.edges" % i].astype(np.int64).tolist()
            for j, r in enumerate(c["results"]):
                for key in ("flags", "flags2"):
                    if "c%d.r%d.%s" % (i, j, key) in z:
                        r[key] = z["c%d.r%d.%s" % (i, j, key)].tobytes().hex()
                for key in ("order_left", "order_left2"):
                    if "c%d.r%d.%s" % (i, j, key) in z:
                        r[key] = z["c%d.r%d.%s" % (i, j, key)].astype(np.int64).tolist()
    return obj
