"""The contract of po_layout_reduce (include/phasm_overlap.h) as plain Python, the seeded
synthetic row sets of tests/golden/reduce_cases.npz, and the loader of that file.

``reduce_edges`` states what the reference's ``remove_transitive_edges`` + ``remove_edges_from`` +
``make_symmetric`` (phasm/assembly_graph.py:182-264, :429-443; phasm/cli/assembler.py:145-159) compute, in the form
the device uses: per node, from its own adjacency list and those of its neighbours.  tests/test_reduce_oracle.py holds
it to every golden case (which the reference's own functions produced); the GPU tests use it where a golden cannot
reach (full-size graphs)."""
import hashlib
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_PARAMS = {"min_read_length": 0, "min_overlap_length": 0, "max_overhang_abs": 1000, "max_overhang_rel": 0.8}
# the last four: comparisons that land on or next to their bound, counted for x that is an IN_PLAY neighbour of v at that moment:
# weight(v,w) + weight(w,x) == limit / == limit + 1 in step 2, weight(w,x) == fuzz / == fuzz - 1 behind position 0 in step 3
BRANCHES = ("step2_eliminations", "step3_first", "step3_fuzz", "step2_skips", "tied_nodes", "asymmetric",
            "step2_at_limit", "step2_just_over", "step3_at_fuzz", "step3_just_under")


# ---- the contract ------------------------------------------------------------------------------------------------

def sorted_adjacency(edges, rank=None):
    """{u: [(v, weight), ...]} ascending by (weight, rank); rank defaults to the position in ``edges`` (the order in
    which the reference's graph first saw each edge)."""
    adj = {}
    for k, (u, v, w) in enumerate(edges):
        adj.setdefault(int(u), []).append((int(w), k if rank is None else int(rank[k]), int(v)))
    return {u: [(v, w) for w, _, v in sorted(l)] for u, l in adj.items()}


def mark_node(v, adj, fuzz, counts=None):
    """The set of w for which edge (v, w) is transitive."""
    nb = adj.get(v)
    if not nb:
        return set()
    in_play = {w for w, _ in nb}
    eliminated = set()
    limit = nb[-1][1] + fuzz
    weights = [wt for _, wt in nb]
    if counts is not None and len(set(weights)) < len(weights):
        counts["tied_nodes"] += 1
    for w, vw in nb:                                    # sequential: the order of nb matters
        if w in eliminated:
            if counts is not None:
                counts["step2_skips"] += 1
            continue
        for x, wx in adj.get(w, ()):
            if x in in_play and x not in eliminated:
                if counts is not None:
                    counts["step2_at_limit"] += vw + wx == limit
                    counts["step2_just_over"] += vw + wx == limit + 1
                if vw + wx <= limit:
                    eliminated.add(x)
                    if counts is not None:
                        counts["step2_eliminations"] += 1
    for w, _ in nb:                                     # every w, whatever became of it
        for pos, (x, wx) in enumerate(adj.get(w, ())):
            if x in in_play and x not in eliminated:
                if counts is not None and pos > 0:
                    counts["step3_at_fuzz"] += wx == fuzz
                    counts["step3_just_under"] += wx == fuzz - 1
                if pos == 0:
                    if counts is not None:
                        counts["step3_first"] += 1
                if wx < fuzz:
                    if counts is not None:
                        counts["step3_fuzz"] += 1
                if pos == 0 or wx < fuzz:
                    eliminated.add(x)
    return eliminated


def reduce_edges(edges, fuzz, rank=None, nodes=None, counts=None):
    """edges: sequence of (u, v, weight[, ...]) with distinct (u, v).  Returns the flag per edge as uint8 (0 kept,
    1 transitive, 2 removed by the symmetry pass).  ``nodes``: mark the out-edges of these nodes only (their flags
    are 0 or 1; no symmetry pass, the other edges get 255)."""
    e3 = [(int(e[0]), int(e[1]), int(e[2])) for e in edges]
    adj = sorted_adjacency(e3, rank)
    index = {(u, v): k for k, (u, v, _) in enumerate(e3)}
    assert len(index) == len(e3), "duplicate edge"
    flags = np.zeros(len(e3), dtype=np.uint8) if nodes is None else np.full(len(e3), 255, dtype=np.uint8)
    for v in (adj if nodes is None else nodes):
        gone = mark_node(v, adj, fuzz, counts)
        for w, _ in adj.get(v, ()):
            flags[index[(v, w)]] = 1 if w in gone else 0
    if nodes is not None:
        return flags
    for (u, v), k in index.items():
        if flags[k] == 1:
            continue
        t = index.get((v ^ 1, u ^ 1))
        if t is None or flags[t] == 1:
            flags[k] = 2
            if counts is not None:
                counts["asymmetric"] += 1
    return flags


def new_counts():
    return {b: 0 for b in BRANCHES}


def degree_profile(edges, fuzz):
    """How the out-degrees of a case meet the thresholds the device code branches on (a wave strides over adj[w] 64
    entries at a time; a node's states leave LDS above 1024 out-edges).  Whatever the fuzz:
    the nodes with 129..1023 out-edges that have a neighbour w with len(adj[w]) > 64; the nodes with more than 1024
    out-edges that have a neighbour w with more than 1024 out-edges, over 64 of whose targets are neighbours too.
    For ``fuzz``: the (v, w) with len(adj[w]) > 128, w IN_PLAY when its turn comes, whose ascending walk meets at least
    one sum within the limit and at least one above it."""
    e3 = [(int(e[0]), int(e[1]), int(e[2])) for e in edges]
    adj = sorted_adjacency(e3)
    out = {"mid_long_w": 0, "wide_pairs": 0, "partial_walks": 0}
    for v, nb in adj.items():
        d = len(nb)
        if d <= 128:
            continue
        in_play = {w for w, _ in nb}
        if d <= 1023:
            out["mid_long_w"] += any(len(adj.get(w, ())) > 64 for w in in_play)
        if d > 1024:
            out["wide_pairs"] += sum(1 for w in in_play if len(adj.get(w, ())) > 1024
                                     and sum(x in in_play for x, _ in adj[w]) > 64)
        eliminated = set()
        limit = nb[-1][1] + fuzz
        for w, vw in nb:
            if w in eliminated:
                continue
            aw = adj.get(w, ())
            within = sum(vw + wx <= limit for _, wx in aw)
            out["partial_walks"] += len(aw) > 128 and 0 < within < len(aw)
            eliminated.update(x for x, wx in aw if x in in_play and vw + wx <= limit)
    return out


# ---- seeded synthetic row sets -------------------------------------------------------------------------------------

def gfa_text(names, lengths, rows):
    out = ["H\tVN:z:2.0\n"]
    for n, l in zip(names, lengths):
        out.append("S\t%s\t%d\t*\n" % (n, l))
    for a, b, s, e, bs, be in rows:
        out.append("E\t*\t%s%s\t%s%s\t%d\t%d\t%d\t%d\t*\n" % (names[a >> 1], "+-"[a & 1], names[b >> 1], "+-"[b & 1], s, e, bs, be))
    return "".join(out)


def line_case(seed, n=40, span=4000, p_keep=0.8, n_false=6, one_way=0.15):
    """Reads laid on a line, some starting at the same position (tied weights), on random strands; a dovetail row for
    most overlapping pairs (a few bases of overhang now and then, so bstart > 0), a second row for some pairs written
    the other way round only now and then, a few false rows between reads that lie far apart (repeat-induced
    edges), lines shuffled."""
    rng = random.Random(seed)
    pos, length, flip = [], [], []
    for i in range(n):
        if i and rng.random() < 0.25:
            pos.append(pos[-1])                       # same start as the read before: equal weights from further left
        else:
            pos.append(rng.randrange(span))
        length.append(rng.randrange(800, 2500))
        flip.append(rng.random() < 0.4)
    order = sorted(range(n), key=lambda i: (pos[i], i))
    rows = []

    def dovetail(i, j, shift_i=0):
        """i's end on j's start, in line coordinates; shift moves the claimed offset (a false or sloppy row)."""
        a, b = 2 * i + flip[i], 2 * j + flip[j]
        ovl = pos[i] + length[i] - pos[j] - shift_i
        oh = rng.choice([0, 0, 0, 3, 17])
        ovl = max(20, min(ovl, length[i] - 1 - 2 * oh, length[j] - 1 - 2 * oh))
        row_f = (a, b, length[i] - ovl - oh, length[i] - oh, oh, oh + ovl)
        # the same alignment read from the other strand: b^1 ends on a^1
        row_r = (b ^ 1, a ^ 1, length[j] - oh - ovl, length[j] - oh, oh, oh + ovl)
        return row_f, row_r

    for x in range(n):
        for y in range(x + 1, n):
            i, j = order[x], order[y]
            if not (pos[i] < pos[j] < pos[i] + length[i] < pos[j] + length[j]):
                continue
            if rng.random() > p_keep:
                continue
            f, r = dovetail(i, j)
            rows.append(f)
            if rng.random() > one_way:
                rows.append(r)                        # (same two edges again: add_edge keeps their place)
    for _ in range(n_false):
        i, j = rng.sample(range(n), 2)
        rows.append(dovetail(i, j, shift_i=rng.randrange(-300, 300))[0])
    rng.shuffle(rows)
    names = ["s%d_%d" % (seed, i) for i in range(n)]
    return names, length, rows


def hub_case(seed, n_nb=5200, n_cross=400):
    """One read with n_nb dovetail neighbours to its right (more than the device keeps in LDS), neighbours that start
    in pairs at the same position, and a few rows among the neighbours."""
    rng = random.Random(seed)
    hub_len = 400_000
    names, length, rows = ["hub"], [hub_len], []
    pos = []
    p = 0
    for k in range(n_nb):
        if k % 7 != 3:
            p += rng.randrange(1, 60)
        pos.append(p)                                  # (k % 7 == 3: the position of the read before)
        names.append("n%d" % k)
        length.append(hub_len - p + 1000 + 13 * k)     # ends behind the hub, each further than the one before
        rows.append((0, 2 * (k + 1), p, hub_len, 0, hub_len - p))
    for _ in range(n_cross):
        i, j = sorted(rng.sample(range(n_nb), 2))
        if pos[i] == pos[j]:
            continue
        ovl = pos[i] + length[i + 1] - pos[j]
        rows.append((2 * (i + 1), 2 * (j + 1), length[i + 1] - ovl, length[i + 1], 0, ovl))
    rng.shuffle(rows)
    return names, length, rows


def stagger_case(seed, n_hubs=3, n_nb=1100, n_cross=300, n_sloppy=80, n_plant=24, plant_fuzz=150):
    """n_hubs long reads three bases apart, each ending ten bases behind the one before, and n_nb neighbours to their
    right as in hub_case: every hub has a row to every later hub and to the neighbours, so an earlier hub v finds a later
    hub w among its neighbours whose list is as long as its own and eliminates nearly all of it.  Not all: every later
    hub claims a larger offset than the true one for n_sloppy of its neighbours (sums above v's limit behind a long run
    within it, one of them by exactly 1 for the last neighbour), and has no row at all to the targets of n_plant rows
    among the neighbours whose weight is plant_fuzz or plant_fuzz - 1 (they survive step 2 and meet step 3's bound)."""
    rng = random.Random(seed)
    hub_len = 400_000
    names = ["hub%d" % h for h in range(n_hubs)]
    length = [hub_len + 7 * h for h in range(n_hubs)]          # hub h lies at 3 h and ends at hub_len + 10 h
    pos, p = [], 3 * n_hubs
    for k in range(n_nb):
        if k % 7 != 3:
            p += rng.randrange(1, 60)
        pos.append(p)
        names.append("n%d" % k)
        length.append(hub_len - p + 1000 + 13 * k)

    def cross(i, j, shift=0):
        ovl = pos[i] + length[n_hubs + i] - pos[j] - shift
        return (2 * (n_hubs + i), 2 * (n_hubs + j), length[n_hubs + i] - ovl, length[n_hubs + i], 0, ovl)

    rows, orphans, planted = [], set(), set()
    for t in range(n_plant):                                   # w -> x at plant_fuzz - (t & 1), behind a shorter row of w
        for _ in range(1000):
            i = rng.randrange(n_nb - 2)
            want = pos[i] + plant_fuzz - (t & 1)
            j = next((j for j in range(i + 2, n_nb) if pos[j] >= want), None)
            if j is not None and pos[j] == want and pos[i + 1] > pos[i] and not {i, i + 1, j} & (orphans | planted):
                break
        else:
            raise AssertionError("no pair of neighbours %d apart" % plant_fuzz)
        rows += [cross(i, i + 1), cross(i, j)]
        planted |= {i, i + 1}
        orphans.add(j)
    for h in range(n_hubs):
        for g in range(h + 1, n_hubs):
            rows.append((2 * h, 2 * g, 3 * (g - h), length[h], 0, length[h] - 3 * (g - h)))
        free = [k for k in range(n_nb - 1) if k not in orphans and k not in planted]
        sloppy = {k: rng.choice([1, 2, 40, rng.randrange(1, 300)]) for k in rng.sample(free, n_sloppy)} if h else {}
        if h:
            sloppy[n_nb - 1] = 1
        for k in range(n_nb):
            if h and k in orphans:
                continue
            a = pos[k] - 3 * h + sloppy.get(k, 0)
            rows.append((2 * h, 2 * (n_hubs + k), a, length[h], 0, length[h] - a))
    for _ in range(n_cross):
        i, j = sorted(rng.sample(range(n_nb), 2))
        if pos[i] == pos[j]:
            continue
        rows.append(cross(i, j, rng.choice([0, 0, 0, rng.randrange(200)])))
    rng.shuffle(rows)
    return names, length, rows


def tie_case(seed, n=8):
    """n groups of reads v, w1, w2, x (and four bystanders): w1 and w2 start at the same place (equal weights from v),
    a sloppy row w1 -> w2 and a sloppy row w2 -> x claim offsets too large for a reduction with fuzz 0 to use, so all
    of v's edges stay.  Reduced AGAIN with a larger fuzz both rows fit under v's limit, and which of the tied w1, w2
    comes first in adj[v] -- the order the graph first saw the two edges, nothing else -- decides whether w2 still
    gets to eliminate x or has been eliminated by w1 before its turn.  (The bystanders y1, y2, z1, z2 take position 0
    of the lists of w1, w2 and of their reverse strands, which step 3 would otherwise use.)"""
    rng = random.Random(seed)
    names, length, rows = [], [], []
    for g in range(n):
        a = rng.randrange(60, 140)
        reads = ("v", "w1", "w2", "x", "y1", "y2", "z1", "z2")
        pos = dict(v=0, w1=a, w2=a, x=a + rng.randrange(280, 320), y1=a + rng.randrange(30, 50), y2=a + rng.randrange(50, 70),
                   z1=rng.randrange(10, 30), z2=rng.randrange(30, 50))
        end = dict(v=1000, w1=1100 + rng.randrange(9), w2=1110 + rng.randrange(9), x=1400, y1=1200, y2=1210, z1=1040, z2=1060)
        base = len(names)
        names += ["t%d_%s" % (g, r) for r in reads]
        length += [end[r] - pos[r] for r in reads]
        for i, j, shift in (("v", "w1", 0), ("v", "w2", 0), ("v", "x", 0), ("w1", "y1", 0), ("w2", "y2", 0), ("z1", "w1", 0),
                            ("z2", "w2", 0), ("w1", "w2", rng.randrange(310, 330)), ("w2", "x", 50)):
            ovl = end[i] - pos[j] - shift
            ni, nj = base + reads.index(i), base + reads.index(j)
            rows.append((2 * ni, 2 * nj, length[ni] - ovl, length[ni], 0, ovl))
            rows.append((2 * nj + 1, 2 * ni + 1, length[nj] - ovl, length[nj], 0, ovl))
    rng.shuffle(rows)
    return names, length, rows


SYNTH = {"line": line_case, "hub": hub_case, "stagger": stagger_case, "tie": tie_case}


# ---- golden file ---------------------------------------------------------------------------------------------------

def pack_flags(flags):
    f = np.asarray(flags, dtype=np.uint8)
    f = np.concatenate([f, np.zeros(-len(f) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (f[:, 0] | (f[:, 1] << 2) | (f[:, 2] << 4) | (f[:, 3] << 6)).astype(np.uint8).tobytes().hex()


def unpack_flags(text, n):
    b = np.frombuffer(bytes.fromhex(text), dtype=np.uint8)
    return np.stack([b & 3, (b >> 2) & 3, (b >> 4) & 3, (b >> 6) & 3], 1).reshape(-1)[:n].astype(np.uint8)


def edge_digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr, dtype="<i8").tobytes()).hexdigest()


def text_digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


def sort_edges(arr):
    """(n, 4) int64 rows (u, v, weight, overlap_len) ordered by (u, v) -- the order the golden's flags are in."""
    arr = np.asarray(arr, dtype=np.int64).reshape(-1, 4)
    return arr[np.lexsort((arr[:, 1], arr[:, 0]))]


def case_text(c):
    """GFA2 text of a golden case."""
    import golden_utils
    import layout_utils
    if "layout_case" in c:      # an inline case of tests/golden/layout_cases.json
        return next(x["text"] for x in layout_utils.load_cases() if x["name"] == c["layout_case"])
    if "synth" in c:            # a seeded row set of this module; the digest proves it is the one the reference saw
        kw = dict(c["synth"])
        kind = kw.pop("kind")
        text = gfa_text(*SYNTH[kind](**kw))
        assert c.get("text_sha256") in (None, text_digest(text)), "synthetic rows drifted from the golden inputs"
        return text
    _, seqs, _, grows = golden_utils.ladder_case(c["ladder"])
    names = ["read%d" % i for i in range(len(seqs) // 2)]
    lengths = [len(seqs[2 * i]) for i in range(len(names))]
    rl = [tuple(int(x) for x in r) for r in grows]
    if c.get("shuffle_seed") is not None:
        random.Random(c["shuffle_seed"]).shuffle(rl)
    return layout_utils.gfa_text(names, lengths, rl)


GOLDEN_FILE = os.path.join(GOLDEN, "reduce_cases.npz")
BULKY = ("stage1", "kept", "flags_by_uv")   # kept as arrays beside the JSON record ("meta") inside the .npz


def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record without its long lists, which go in as arrays ("c<case>.stage1",
    "c<case>.f<fuzz>.kept" int32, "c<case>.f<fuzz>.flags" packed bytes).  Written entry by entry with a fixed date, so
    the same content gives the same bytes."""
    import io
    import zipfile
    arrays, meta = {}, json.loads(json.dumps(obj))
    for i, c in enumerate(meta["cases"]):
        if "stage1" in c:
            arrays["c%d.stage1" % i] = np.asarray(c.pop("stage1"), dtype="<i4").reshape(-1, 4)
        for fuzz, r in c["results"].items():
            arrays["c%d.f%s.flags" % (i, fuzz)] = np.frombuffer(bytes.fromhex(r.pop("flags_by_uv")), dtype=np.uint8)
            if "kept" in r:
                arrays["c%d.f%s.kept" % (i, fuzz)] = np.asarray(r.pop("kept"), dtype="<i4").reshape(-1, 4)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def load_golden(path=GOLDEN_FILE):
    """The record save_golden was given: {"branch_totals": ..., "cases": [...]}, long lists back in place."""
    with np.load(path) as z:
        obj = json.loads(z["meta"].tobytes().decode())
        for i, c in enumerate(obj["cases"]):
            if "c%d.stage1" % i in z:
                c["stage1"] = z["c%d.stage1" % i].astype(np.int64).tolist()
            for fuzz, r in c["results"].items():
                r["flags_by_uv"] = z["c%d.f%s.flags" % (i, fuzz)].tobytes().hex()
                if "c%d.f%s.kept" % (i, fuzz) in z:
                    r["kept"] = z["c%d.f%s.kept" % (i, fuzz)].astype(np.int64).tolist()
    return obj


def case_stage1(c):
    """Stage-1 edges of a case as the reference built them, in its graph's insertion order ((n, 4) int64), or None
    where the golden holds their digest only."""
    return np.asarray(c["stage1"], dtype=np.int64).reshape(-1, 4) if "stage1" in c else None
