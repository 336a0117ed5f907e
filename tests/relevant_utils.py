"""The relevant reads of a bubble of `phasm phase` (po_phase_index, po_phase_relevant): the cases, a plain dict-of-dicts
``definition``, and the goldens recorded from the reference's own methods (tests/golden/make_relevant_golden.py).

A CASE: ``n_seg`` segments -- segment i has the oriented reads 2i (``s<i>+``) and 2i + 1 (``s<i>-``) of length ``lengths[i]`` --
the rows ``(a, b, astart, aend, bstart, bend)`` over oriented ids in ``rows_flat``, and QUERIES: ``cur_graph``, ``prev_graph``,
``prev_aligning``, ``preds`` (``[read, edge_len]`` of the predecessors of the exit that are plain reads), ``mode`` (0 = spanning,
1 = all) and ``min_span``.  The golden stub graph also gives every exit a MergedReads predecessor, which must yield len(read).

A RESULT of a query: ``cur_aligning``, ``n_spanning``, ``fell_back``, ``rel_reads``, ``overlap_max``, ``aln_off``, ``aln_y`` (GLOBAL
ids, ascending per read), ``aln_a0``, ``aln_a1``, ``b_reads``.  All integers: every comparison is exact."""
import os

import numpy as np

import components_utils as cu
import reduce_utils as ru

GOLDEN_FILE = os.path.join(ru.GOLDEN, "relevant_cases.npz")
RESULT_KEYS = ("cur_aligning", "n_spanning", "fell_back", "rel_reads", "overlap_max", "aln_off", "aln_y", "aln_a0", "aln_a1", "b_reads")
HUB_DEGREES = (1, 63, 64, 65, 257, 2049)   # 2049: a segment that nine workgroups of 256 threads sort by rank


def rows_of(case):
    return np.asarray(case["rows_flat"], dtype=np.int64).reshape(-1, 6)


def lengths_of(case):
    """The length of every oriented read id."""
    return np.repeat(np.asarray(case["lengths"], dtype=np.int64), 2)


# ---- the definition: the reference's loops on plain dicts -----------------------------------------------------------------------

def mapping(case):
    """``_get_read_alignments`` (assembler.py:313-328): m[x][y] = (a0, a1, seq); a later write replaces an earlier one."""
    m = {}
    for i, (a, b, astart, aend, bstart, bend) in enumerate(rows_of(case).tolist()):
        m.setdefault(a, {})[b] = (astart, aend, 2 * i)
        m.setdefault(b, {})[a] = (bstart, bend, 2 * i + 1)
    return m


def index_definition(case):
    """(offsets, entries as (b, a0, a1, seq) tuples) in ascending (x, y)."""
    m, n_ids = mapping(case), 2 * case["n_seg"]
    off, entries = [0], []
    for x in range(n_ids):
        entries += [(y,) + m[x][y] for y in sorted(m.get(x, {}))]
        off.append(len(entries))
    return off, entries


def definition(case, q, m=None):
    m = mapping(case) if m is None else m
    length = lengths_of(case)
    cur, prev_graph, prev_aligning = set(q["cur_graph"]), set(q["prev_graph"]), set(q["prev_aligning"])
    empty = {k: [] for k in RESULT_KEYS}
    empty.update(n_spanning=0, fell_back=0, aln_off=[0])
    if not cur:
        return empty
    cur_aligning = set(cur)                                  # get_aligning_reads (phasing.py:541-550)
    for x in cur:
        cur_aligning.update(m.get(x, {}))
    spanning = prev_aligning & cur_aligning                  # phasing.py:263-264
    fell_back = q["mode"] == 0 and len(spanning) < q["min_span"]
    if fell_back:                                            # new_block(): phasing.py:353-356
        prev_graph = set()
    relevant = cur_aligning if (q["mode"] == 1 or fell_back) else spanning
    G = sorted(cur | prev_graph)
    out = dict(empty, cur_aligning=sorted(cur_aligning), n_spanning=len(spanning), fell_back=int(fell_back), rel_reads=sorted(relevant),
               b_reads=G)
    out["overlap_max"], out["aln_off"], out["aln_y"], out["aln_a0"], out["aln_a1"] = [], [0], [], [], []
    for r in sorted(relevant):                               # get_relevant_read_info (phasing.py:366-404)
        for y in sorted(m.get(r, {})):
            if y in cur or y in prev_graph:
                out["aln_y"].append(y)
                out["aln_a0"].append(m[r][y][0])
                out["aln_a1"].append(m[r][y][1])
        out["aln_off"].append(len(out["aln_y"]))
        om = int(length[r])
        for p, edge_len in q["preds"]:                       # _get_max_possible_overlap (phasing.py:406-419)
            if p in m and r in m[p]:
                om = min(om, edge_len - m[p][r][0])
        out["overlap_max"].append(om)
    return out


def result_of_relevant(rel):
    """A ``phasm_amd.phasing.RelevantReads`` as a RESULT."""
    b = np.asarray(rel.b_reads, dtype=np.int64)
    return {"cur_aligning": rel.cur_aligning.tolist(), "n_spanning": int(rel.n_spanning), "fell_back": int(rel.fell_back),
            "rel_reads": rel.rel_reads.tolist(), "overlap_max": rel.overlap_max.tolist(), "aln_off": rel.aln_off.tolist(),
            "aln_y": b[np.asarray(rel.aln_b, dtype=np.int64)].tolist() if len(rel.aln_b) else [], "aln_a0": rel.aln_a0.tolist(),
            "aln_a1": rel.aln_a1.tolist(), "b_reads": rel.b_reads.tolist()}


def same_result(got, want, where=""):
    for key in RESULT_KEYS:
        g, w = got[key], want[key]
        g = g.tolist() if hasattr(g, "tolist") else g
        w = w.tolist() if hasattr(w, "tolist") else w
        assert g == w, "%s: %s differs" % (where, key)


def query_source(src, index, q):
    """A query through anything with ``phase_relevant`` (an ExactOverlapper, a HostIndex)."""
    return result_of_relevant(src.phase_relevant(index, q["cur_graph"], q["prev_graph"], q["prev_aligning"], [tuple(p) for p in q["preds"]],
                                                 q["mode"], q["min_span"]))


def golden_index(case):
    """(offsets, entries) of a golden case, the entries as (b, a0, a1, seq) tuples."""
    return case["index_off"], list(zip(case["index_b"], case["index_a0"], case["index_a1"], case["index_seq"]))


def same_index(off, entries, want_off, want_entries):
    """``off`` / ``entries``: what ``phase_index_entries`` gives (offsets, structured b, a0, a1, seq)."""
    assert np.asarray(off).astype(np.int64).tolist() == [int(v) for v in want_off]
    assert [tuple(int(v) for v in e) for e in entries.tolist()] == [tuple(int(v) for v in w) for w in want_entries]


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def _q(cur, prev_graph=(), prev_aligning=(), preds=(), mode=0, min_span=0):
    return {"cur_graph": list(cur), "prev_graph": list(prev_graph), "prev_aligning": list(prev_aligning),
            "preds": [list(p) for p in preds], "mode": mode, "min_span": min_span}


def _case(name, lengths, rows, queries):
    flat = [int(v) for row in rows for v in row]
    return {"name": name, "n_seg": len(lengths), "lengths": list(lengths), "rows_flat": flat, "queries": queries}


def case_writes():
    """Which write wins: duplicate rows, (a, b) then (b, a), a self row, x+ and x-, a read with no row."""
    rows = [(0, 2, 1, 10, 2, 11), (0, 2, 3, 12, 4, 13),           # duplicate (a, b): the later one wins
            (4, 6, 5, 50, 6, 60), (6, 4, 7, 70, 8, 80),           # (a, b) then (b, a): the later row wins under both keys
            (8, 8, 1, 5, 2, 9),                                   # a self row: (bstart, bend) stays
            (10, 12, 1, 2, 3, 4), (11, 12, 5, 6, 7, 8),           # x+ and x-: two keys
            (0, 4, 9, 19, 8, 18), (2, 0, 21, 31, 22, 32)]         # (2, 0) replaces both writes of the first two rows
    qs = [_q([0, 4, 8, 10, 11, 14], mode=1),                      # 14: an interior read with no row at all
          _q([8], mode=1), _q([12], prev_graph=[10, 11], mode=1),
          _q([0], prev_graph=[2, 4], prev_aligning=[2, 4, 6], mode=0, min_span=2)]
    return _case("writes", [100 + 3 * i for i in range(9)], rows, qs)    # 18 ids


def case_bubble():
    """One bubble: interior 20, 22, 24 (26 has no row), previous bubbles 10, 12, entrance 30, exit 32, downstream 34; the
    aligning reads 40 .. 52.  Every predecessor situation, duplicates in every list, the empty sets, the fallback edge."""
    L = [200] * 30
    L[21] = 90                                                    # reads 42 / 43 are short
    rows = [(40, 20, 5, 105, 0, 100), (40, 10, 0, 50, 10, 60), (40, 30, 1, 2, 3, 4), (40, 32, 110, 150, 0, 40), (40, 34, 160, 190, 0, 30),
            (22, 42, 0, 80, 3, 83), (42, 12, 2, 30, 40, 68), (42, 24, 50, 88, 0, 38),
            (44, 24, 10, 60, 0, 50), (46, 22, 0, 100, 20, 120), (46, 20, 30, 130, 0, 100), (48, 10, 0, 10, 0, 10),
            (50, 20, 7, 70, 0, 63), (50, 50, 11, 60, 13, 62),     # 50 also aligns to itself
            (28, 40, 120, 180, 15, 75),                           # pred 28 -> read 40: a0(28, 40) = 120
            (28, 42, 170, 190, 0, 20), (36, 42, 30, 60, 10, 40),  # two preds on read 42
            (38, 44, 300, 310, 0, 10),                            # a0 above any edge_len: negative
            (52, 52, 3, 9, 4, 10), (52, 24, 0, 5, 0, 5)]          # 52 is pred AND relevant read, through its self row
    cur, pg, pa = [20, 22, 24, 26], [10, 12], [40, 42, 44, 48, 56]
    qs = [_q(cur, pg, pa, [], 0, 2),                              # no pred
          _q(cur, pg, pa, [(54, 150)], 0, 2),                     # a pred without an alignment to any read
          _q(cur, pg, pa, [(28, 250)], 0, 2),                     # 250 - 120 = 130 < len(40) = 200; 250 - 170 = 80 < len(42) = 90
          _q(cur, pg, pa, [(28, 120)], 0, 2),                     # 0 for read 40, negative for 42
          _q(cur, pg, pa, [(38, 100)], 0, 2),                     # negative for 44
          _q(cur, pg, pa, [(28, 1000)], 0, 2),                    # more than len: len stays
          _q(cur, pg, pa, [(28, 250), (36, 100)], 0, 2),          # two: the minimum (42: min(80, 70))
          _q(cur, pg, pa, [(36, 100), (28, 250)], 0, 2),
          _q(cur, pg, [40, 52], [(52, 20)], 0, 1),                # the pred equal to the read: 20 - a0(52, 52) = 20 - 4
          _q(cur + cur[::-1], pg + pg, pa + pa, [(28, 250), (28, 250)], 0, 2),   # duplicates in every list
          _q([], pg, pa, [(28, 250)], 0, 0), _q([], [], [], [], 1, 0),           # an empty cur_graph
          _q(cur, [], [], [], 0, 0), _q(cur, [], [], [], 0, 1),   # empty prev sets in mode 0
          _q(cur, pg, pa, [(28, 250)], 0, 3),                     # n_spanning (3: 40, 42, 44) == min_spanning_reads
          _q(cur, pg, pa, [(28, 250)], 0, 4),                     # one below: the fallback
          _q(cur, pg, pa, [(28, 250)], 1, 9)]                     # mode 1 ignores min_spanning_reads
    return _case("bubble", L, rows, qs)                           # 60 ids


def case_ids():
    """Read ids 31, 32, 33, 63, 64, 65 and the highest id in every set; n_ids = 134 is no multiple of 64 (nor of 32)."""
    n_seg = 67
    edge = [31, 32, 33, 63, 64, 65, 133]
    rows = []
    for k, x in enumerate(edge):
        for j, y in enumerate(edge):
            if (k + j) % 3 != 2:
                rows.append((x, y, k, 10 * k + j + 20, j, 10 * j + k + 20))
    rows += [(0, 31, 1, 9, 2, 10), (133, 1, 3, 8, 4, 9)]
    qs = [_q(edge, edge, edge, [(e, 40 + e) for e in edge], 0, 1), _q(edge, edge, edge, [(133, 25)], 1, 0),
          _q([133], [31, 65], [33, 63, 64, 133], [(31, 30), (65, 22)], 0, 1), _q([0], [31], [31], [], 0, 1)]
    return _case("ids", [50 + i for i in range(n_seg)], rows, qs)


def case_degrees():
    """Hub reads with 1, 63, 64, 65, 257 and 2049 entries; the hubs as cur_graph (their segments marked), as relevant reads
    (their segments counted and written, past one wave's step of 64) and as preds."""
    n_seg = 1237                                                  # 2474 ids: 77 words of 32 and 10 left over
    hubs = {h: d for h, d in zip((3, 70, 141, 200, 333, 2473), HUB_DEGREES)}
    rows, first = [], []
    for h, d in hubs.items():
        ys = [y for y in range(2474) if y not in hubs][:d] if d > 300 else [(h * 7 + 5 * j) % 2474 for j in range(3 * d)]
        ys = [y for y in dict.fromkeys(ys) if y not in hubs][:d]
        assert len(ys) == d
        first.append(ys[0])
        for j, y in enumerate(ys):
            rows.append((h, y, j, j + 100, 2 * j, 2 * j + 100) if j % 3 else (y, h, 2 * j, 2 * j + 100, j, j + 100))
    every = list(range(0, 2474, 2)) + [first[3], first[4]]
    qs = [_q(list(hubs), preds=[(2473, 500), (3, 40)], mode=1),                  # every hub's segment marked; the hubs as preds
          _q(first + [4, 6], every, list(hubs), [(2473, 500), (3, 40)], 0, 6),   # all six hubs relevant, G wide: long alignment lists
          _q([0, 1, 2], list(hubs), [2473], [(333, 77)], 0, 1)]
    return _case("degrees", [120 + (i % 7) for i in range(n_seg)], rows, qs)


SPECS = {"writes": case_writes, "bubble": case_bubble, "ids": case_ids, "degrees": case_degrees}


def union_case(cases, n_copies):
    """Disjoint copies of the small cases behind one another (ids shifted per copy): (lengths per segment, rows [n, 6], the id
    shift of every (copy, case))."""
    lengths, rows, shifts, seg = [], [], [], 0
    blocks = [(c["lengths"], rows_of(c)) for c in cases]
    for _ in range(n_copies):
        for ln, rw in blocks:
            shift = 2 * seg
            shifted = rw.copy()
            shifted[:, :2] += shift
            rows.append(shifted)
            lengths += ln
            shifts.append(shift)
            seg += len(ln)
    return lengths, np.concatenate(rows), shifts


def shifted_query(q, shift):
    out = dict(q)
    for key in ("cur_graph", "prev_graph", "prev_aligning"):
        out[key] = [v + shift for v in q[key]]
    out["preds"] = [[p + shift, e] for p, e in q["preds"]]
    return out


def shifted_result(res, shift):
    out = dict(res)
    for key in ("cur_aligning", "rel_reads", "aln_y", "b_reads"):
        out[key] = [v + shift for v in (res[key].tolist() if hasattr(res[key], "tolist") else res[key])]
    return out


def add_reads(ov, lengths):
    for i, n in enumerate(lengths):
        ov.add_segment("s%d" % i, int(n))


def rows_array(rows):
    from phasm_amd._lib import ROW_DTYPE
    out = np.zeros(len(rows), dtype=ROW_DTYPE)
    for k, name in enumerate(ROW_DTYPE.names):
        out[name] = np.asarray(rows)[:, k] if len(rows) else 0
    return out


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]


# ---- a phase golden (tests/phase_utils.py) as rows and one query: the chain index -> gather -> bubble -> branch ----------------

BIG_LEN, PRED_EDGE = 1000000, 500000


def phase_case_as_rows(pc):
    """A bubble of phase_cases.npz as reads, rows and a query whose gather gives the bubble back: local b read b is oriented id
    2b, relevant read r is 2(n_b + r), one predecessor 2(n_b + R) aligned to every relevant read at PRED_EDGE - overlap_max[r],
    so that overlap_max comes out of the minimum (every read is BIG_LEN long).  Relevant reads without an alignment join
    cur_graph: they must be aligning reads, and as b reads that no alignment names they change no score.  None when a read of
    the bubble has two alignments to one b read (one key: the index keeps one)."""
    n_b, R = pc["n_b"], pc["R"]
    rid = lambda r: 2 * (n_b + r)   # noqa: E731
    pred = 2 * (n_b + R)
    rows, bare = [], []
    for r in range(R):
        lo, hi = pc["aln_off"][r], pc["aln_off"][r + 1]
        bs = list(pc["aln_b"][lo:hi])
        if len(set(bs)) != len(bs) or not -BIG_LEN < pc["overlap_max"][r] <= PRED_EDGE:
            return None
        if not bs:
            bare.append(rid(r))
        for j in range(lo, hi):
            rows.append((rid(r), 2 * pc["aln_b"][j], pc["aln_a0"][j], pc["aln_a1"][j], 0, pc["aln_a1"][j] - pc["aln_a0"][j]))
        rows.append((pred, rid(r), PRED_EDGE - pc["overlap_max"][r], PRED_EDGE, 0, 1))
    k, P, C = pc["k"], pc["P"], pc["C"]
    glob = lambda ids: [2 * int(b) for b in ids]   # noqa: E731
    return {"lengths": [BIG_LEN] * (n_b + R + 1), "rows": np.asarray(rows, dtype=np.int64).reshape(-1, 6),
            "cur_graph": [2 * b for b in range(n_b)] + bare, "prev_aligning": [rid(r) for r in range(R)], "preds": [(pred, PRED_EDGE)],
            "paths": [glob(pc["path_ids"][pc["path_off"][p]:pc["path_off"][p + 1]]) for p in range(P)],
            "read_sets": [[glob(pc["set_ids"][pc["set_off"][c * k + i]:pc["set_off"][c * k + i + 1]]) for i in range(k)] for c in range(C)]}


def chained_case(pc, bubble):
    """The phase case with the arrays of a bubble that came out of the chain."""
    import phase_utils as pu
    again = dict(pc)
    for key in pu.INPUT_KEYS:
        again[key] = getattr(bubble, key).tolist()
    again["n_b"], again["R"] = bubble.n_b, bubble.n_reads
    return again


def chain_cases(n=3):
    """The first n phase goldens with relevant reads, a prune step and a kept list that the chain can carry."""
    import phase_utils as pu
    out = []
    for pc in pu.load_golden()["cases"]:
        if pc["R"] >= 2 and pc["prune"] is not None and len(pc["ref"]["kept_rl"]) >= 2 and phase_case_as_rows(pc) is not None:
            out.append(pc)
        if len(out) == n:
            break
    assert len(out) == n
    return out
