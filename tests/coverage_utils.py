"""The contract of po_layout_coverage (include/phasm_overlap.h) as plain Python, the scheme the
kernels use, seeded generators and the loader of tests/golden/coverage_cases.npz.

``edge_coverage`` states what the reference's ``average_coverage_path(g, read_alignments, [u, v])``
(phasm/assembly_graph.py:544-591; phasm/cli/assembler.py:190-193) computes for every edge.  ``edge_coverage_by_sets`` gets
there the way the device does (phasm_amd/csrc/coverage.hip.h): one set of aligning reads per graph node with its sum, then
inclusion-exclusion over the shorter of the two sets of an edge.  tests/test_coverage_oracle.py holds both to every golden
application, which the reference's own function produced (tests/golden/make_coverage_golden.py)."""
import json
import os
import random

import numpy as np

import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu

GOLDEN_FILE = os.path.join(ru.GOLDEN, "coverage_cases.npz")
SITUATIONS = ("contained_read_counts", "dropped_row_counts", "one_strand_only", "duplicate_rows", "self_row", "common_reads",
              "no_common_read", "merged_self_loops", "path_over_64_members", "set_over_1024_reads", "sum_over_2_32",
              "path_length_over_2_31", "zero_length_segments")


def new_counts():
    return {s: 0 for s in SITUATIONS}


def aligning_reads(rows):
    """A(x) per oriented read x: every read that shares a row with x, in either position (alignment_recorder,
    assembler.py:65-76: ``read_alignments[a][b]`` and ``[b][a]`` for EVERY line, before any filter)."""
    A = {}
    for r in np.asarray(rows, dtype=np.int64).reshape(-1, 6)[:, :2].tolist():
        a, b = r
        A.setdefault(a, set()).add(b)
        A.setdefault(b, set()).add(a)
    return A


def _members_of(members, n):
    return members.get(int(n), [int(n)]) if members else [int(n)]


def edge_coverage(rows, edges, members, lengths):
    """rows: (a, b, ...) per alignment; edges: (u, v, weight, overlap_len); members: {merged node: its reads}; lengths:
    the length of every node id, merged nodes included.  Returns (read_length_sum, path_length) as int64 arrays and the
    quotients as a float64 array, in the order of ``edges`` -- average_coverage_path, line by line."""
    A = aligning_reads(rows)
    sums, paths, avg = [], [], []
    for u, v, w, _ in np.asarray(edges, dtype=np.int64).reshape(-1, 4).tolist():
        path_length = w                                   # node_path_edges([u, v]) yields (u, v, weight) once
        aligning = set()
        for m in _members_of(members, u):
            aligning |= A.get(m, set())
        if lengths[v]:                                    # `if include_last and last:` -- a read's bool is its length
            path_length += int(lengths[v])
            for m in _members_of(members, v):
                aligning |= A.get(m, set())
        sums.append(sum(int(lengths[r]) for r in aligning))
        paths.append(path_length)
        avg.append(sums[-1] / path_length)                # ZeroDivisionError as the reference raises it
    return np.asarray(sums, dtype=np.int64), np.asarray(paths, dtype=np.int64), np.asarray(avg, dtype=np.float64)


def node_sets(rows, edges, members):
    """The per-node sets of the device's scheme: {node with an edge: the distinct reads aligning to one of its members}."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    used = set(e[:, 0].tolist()) | set(e[:, 1].tolist())
    node_of = {}
    for n in used:
        for m in _members_of(members, n):
            node_of[m] = n
    sets = {n: set() for n in used}
    for a, b in np.asarray(rows, dtype=np.int64).reshape(-1, 6)[:, :2].tolist():
        for x, y in ((a, b), (b, a)):
            if x in node_of:
                sets[node_of[x]].add(y)
    return sets


def set_stats(rows, edges, members):
    """(n_nodes, n_pairs, max_set) of po_coverage_stats."""
    sets = node_sets(rows, edges, members)
    return len(sets), sum(len(s) for s in sets.values()), max([len(s) for s in sets.values()] + [0])


def edge_coverage_by_sets(rows, edges, members, lengths, counts=None):
    """The same by the device's scheme: sum[node] over its set; per edge sum[u] + sum[v] - the lengths of the reads of the
    shorter set that are in the other one too; u == v takes sum[u] alone; a v of length 0 takes sum[u] alone."""
    sets = node_sets(rows, edges, members)
    total = {n: sum(int(lengths[r]) for r in s) for n, s in sets.items()}
    sums, paths = [], []
    for u, v, w, _ in np.asarray(edges, dtype=np.int64).reshape(-1, 4).tolist():
        lv = int(lengths[v])
        s = total[u]
        if u != v and lv:
            a, b = (u, v) if len(sets[u]) <= len(sets[v]) else (v, u)
            both = [y for y in sets[a] if y in sets[b]]
            s += total[v] - sum(int(lengths[y]) for y in both)
            if counts is not None:
                counts["common_reads" if both else "no_common_read"] += 1
        sums.append(s)
        paths.append(w + lv)
    sums, paths = np.asarray(sums, dtype=np.int64), np.asarray(paths, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):                      # (a zero path: the plain statement raises)
        return sums, paths, sums.astype(np.float64) / paths.astype(np.float64)


# ---- seeded text cases: each aimed at one way the kernels can go wrong ---------------------------------------------------

def dovetail(u, v, w, lu, lv):
    """The row of an exact dovetail of u's suffix on v's prefix, u starting w bases before v: edge (u, v, weight w)."""
    ovl = min(lu - w, lv)
    return (u, v, w, w + ovl, 0, ovl)


def mirror(row, lengths):
    """The same alignment seen from the other strand: (b^1, a^1) with both ranges reversed."""
    a, b, s, e, bs, be = row
    la, lb = lengths[a >> 1], lengths[b >> 1]
    return (b ^ 1, a ^ 1, lb - be, lb - bs, la - e, la - s)


def mix_case(seed, n=36, n_small=24):
    """A line of reads with rows to the next and the second next read (the two ends of an edge share aligning reads), most
    of them written on ONE strand only (the mirror node has no aligning read of its own), some twice; small reads contained
    in a line read, each with a dovetail row of its own that the removal of contained reads drops; rows with a large
    overhang that MaxOverhang drops; a read with a row onto itself; a component of two reads (no common aligning read)."""
    rng = random.Random(7000 + seed)
    L = tu.READ_LEN
    names = ["m%d_%d" % (seed, i) for i in range(n + 2 + n_small)]
    lengths = [L] * (n + 2) + [3000] * n_small
    rows = []
    for i in range(n - 1):
        w1 = rng.randrange(3000, 6000)
        rows.append(dovetail(2 * i, 2 * i + 2, w1, L, L))
        if i + 2 < n:
            rows.append(dovetail(2 * i, 2 * i + 4, w1 + rng.randrange(3000, 6000), L, L))
    rows += [mirror(r, lengths) for r in rows if rng.random() < 0.4]
    rows += [r for r in rows if rng.random() < 0.15]                           # duplicate E lines
    for i in range(0, n - 6, 5):                                               # MaxOverhang drops these
        rows.append((2 * i + (i & 1), 2 * (i + 5), 5000, 9000, 6000, 10000))
    x = 2 * rng.randrange(4, n - 4)
    rows.append((x, x, 700, L, 0, L - 700))                                    # a read that overlaps itself
    rows.append(dovetail(2 * n, 2 * n + 2, 4000, L, L))                        # two reads on their own
    for k in range(n_small):                                                   # contained reads
        c, host = 2 * (n + 2 + k), 2 * rng.randrange(n)
        s = rng.randrange(1000, L - 4000)
        rows.append((host, c, s, s + 3000, 0, 3000))
        other = 2 * rng.randrange(n) + 1
        rows.append((c ^ (k & 1), other, 1000, 3000, 0, 2000))                 # a dovetail of the contained read
    rng.shuffle(rows)
    return names, lengths, rows


def stem_case(seed, stem=80, branch=7, n_small=1700, length=None, weight=None, prefix="y"):
    """A stem of reads that forks into two branches (no tips: more than 5000 bases each), every row on both strands: after
    cleaning the stem is one merged node of ``stem`` members with two out-edges.  ``n_small`` small reads lie inside one
    read of the stem: that read, and the merged node, have more than ``n_small`` aligning reads."""
    rng = random.Random(8000 + seed)
    L = length or tu.READ_LEN
    n = stem + 2 * branch
    names = ["%s%d_%d" % (prefix, seed, i) for i in range(n + n_small)]
    lengths = [L] * n + [400] * n_small
    wt = (lambda: weight) if weight else (lambda: rng.randrange(3000, 6000))
    chain = list(range(stem))
    pairs = list(zip(chain, chain[1:]))
    for b in range(2):
        br = [stem - 1] + [stem + b * branch + i for i in range(branch)]
        pairs += list(zip(br, br[1:]))
    rows = [dovetail(2 * a, 2 * b, wt(), L, L) for a, b in pairs]
    rows += [mirror(r, lengths) for r in rows]
    host = 2 * (stem // 2)
    for k in range(n_small):
        s = rng.randrange(100, L - 1000)
        r = (host, 2 * (n + k) + (k & 1), s, s + 400, 0, 400)
        rows.append(r if k % 3 else mirror(r, lengths))
    rng.shuffle(rows)
    return names, lengths, rows


def giant_case(seed):
    """Segments of 2 000 000 000 bases 200 000 000 apart: three of them align to one node (the sum passes 2**32) and
    weight + len(v) passes 2**31."""
    return stem_case(seed, stem=3, branch=3, n_small=0, length=2000000000, weight=200000000, prefix="g")


def zero_case(seed, n=12):
    """The probe for an edge into a segment of length 0: a line of reads and two empty segments with rows of every shape an
    empty range allows.  Stage 1 classifies each of them as a containment of the empty segment (alignments.py:248-258: with
    len 0 both its start and its remainder are 0, never larger than the other read's), so no edge can reach one."""
    rng = random.Random(9000 + seed)
    L = tu.READ_LEN
    names = ["z%d_%d" % (seed, i) for i in range(n + 2)]
    lengths = [L] * n + [0, 0]
    rows = [dovetail(2 * i, 2 * i + 2, rng.randrange(3000, 6000), L, L) for i in range(n - 1)]
    rows += [mirror(r, lengths) for r in rows]
    z0, z1 = 2 * n, 2 * n + 2
    rows += [(4, z0, L, L, 0, 0), (z0, 6, 0, 0, 0, 0), (8, z0 + 1, 0, 0, 0, 0), (z1, 10, 0, 0, L, L), (12, z1, 500, 500, 0, 0),
             (z1 + 1, z0, 0, 0, 0, 0)]
    rng.shuffle(rows)
    return names, lengths, rows


SYNTH = {"mix": mix_case, "stem": stem_case, "giant": giant_case, "zero": zero_case}
NEW_CASES = ({"kind": "mix", "seed": 1}, {"kind": "mix", "seed": 2}, {"kind": "stem", "seed": 1}, {"kind": "giant", "seed": 1},
             {"kind": "zero", "seed": 1})


def case_text(c):
    """GFA2 text of a golden case: the cases of this module by seed, everything else through merge_utils."""
    kind = c.get("synth", {}).get("kind")
    if kind in SYNTH:
        kw = dict(c["synth"])
        text = ru.gfa_text(*SYNTH[kw.pop("kind")](**kw))
        assert c.get("text_sha256") in (None, ru.text_digest(text)), "synthetic rows drifted from the golden inputs"
        return text
    return mu.case_text(c)


# ---- golden file -----------------------------------------------------------------------------------------------------

_ARRAYS = (("u", "<u4"), ("v", "<u4"), ("read_length_sum", "<u8"), ("path_length", "<i8"), ("avg_coverage", "<f8"))
DIGEST_ABOVE = 3000   # edges: a larger application is kept as the digest of its five arrays


def arrays_digest(u, v, sums, paths, avg):
    import hashlib
    h = hashlib.sha256()
    for a, (_, dt) in zip((u, v, sums, paths, avg), _ARRAYS):
        h.update(np.ascontiguousarray(np.asarray(a).astype(dt)).tobytes())
    return h.hexdigest()


def check_record(rec, u, v, sums, paths, avg):
    """(u, v, read_length_sum, path_length, avg_coverage) in (u, v) order against one golden record: the arrays where the
    file holds them, their digest for the large applications.  Integers with ==, the float64 quotients bit for bit."""
    assert len(u) == rec["n_edges"]
    if "sha256" in rec:
        assert arrays_digest(u, v, sums, paths, avg) == rec["sha256"]
        return
    assert np.asarray(u).tolist() == rec["u"].tolist() and np.asarray(v).tolist() == rec["v"].tolist()
    assert np.asarray(sums).tolist() == rec["read_length_sum"].tolist()
    assert np.asarray(paths).tolist() == rec["path_length"].tolist()
    assert np.asarray(avg, dtype=np.float64).tobytes() == rec["avg_coverage"].tobytes()


def save_golden(obj, path=GOLDEN_FILE):
    """One .npz: "meta" = the JSON record; beside it per application the five arrays, in (u, v) order -- or, above
    DIGEST_ABOVE edges, their digest in the record."""
    import io
    import zipfile
    arrays = {}
    for i, c in enumerate(obj["cases"]):
        for j, r in enumerate(c["results"]):
            if "sha256" in r:
                continue
            held = [np.asarray(r.pop(key), dtype=dt) for key, dt in _ARRAYS]
            if r["n_edges"] > DIGEST_ABOVE:
                r["sha256"] = arrays_digest(*held)
                continue
            for (key, _), a in zip(_ARRAYS, held):
                arrays["c%d.r%d.%s" % (i, j, key)] = a
    meta = json.loads(json.dumps(obj))
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
            for j, r in enumerate(c["results"]):
                for key, _ in _ARRAYS:
                    if "sha256" not in r:
                        r[key] = z["c%d.r%d.%s" % (i, j, key)]
    return obj
