"""Deterministic read sets for the inexact extension mode (``po_overlaps_ex``, ``max_diff > 0``), shared by the CPU test
of the restatement (tests/test_extend_definition.py) and the GPU test of the kernels (tests/test_gpu_extend_edges.py).

A case is ``(name, seqs, min_length, max_diff, band, expect)``.  ``expect`` is ``None`` or the list of rows known BY
CONSTRUCTION: each builder says in one sentence why its rows are what they are; nothing here is computed by a DP.

Constructed pairs are ``a = U + X [+ ...]`` and ``b = Y + ...``: U is ``p`` random bases (the anchor position), X random
bases, Y a copy of X with the edits the case is about, never inside the first 32 bases (the anchor K-mer is exact).
With ``p >= 1`` and random U, a's own prefix K-mer does not occur in b: the pair (b, a) has no candidate.
Rows are ``(a, b, astart, aend, 0, bend)``; ``x = a[p:]`` (``rem`` bases), ``y = b`` (``lb`` bases); row i of the DP
consumes ``x[i - 1]``.
"""
from __future__ import annotations

import numpy as np

M = 40                                                   # min_length of the constructed pairs (anchor = 32 bases)
P_SWEEP = list(range(1, 17)) + [63, 64, 65]              # every p mod 16; p mod 64 in {63, 0, 1}
W_SWEEP = [1, 4, 5, 8, 9, 15, 16, 30]
RC = bytes.maketrans(b"ACGT", b"TGCA")


def rnd(n, *seed):
    """n random bases; the same seed gives the same bases, different seeds unrelated ones."""
    rng = np.random.default_rng([int(s) for s in seed])
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=n))


def with_subs(x, positions):
    """x with the base at every position replaced by one that differs from x[q - 1], x[q] and x[q + 1]: the new base matches
    nothing one diagonal away either, so neighbouring substitutions cannot be had cheaper through a pair of indels."""
    y = bytearray(x)
    for q in positions:
        assert q >= 32, "the anchor K-mer stays exact"
        y[q] = next(c for c in b"ACGT" if c not in x[max(q - 1, 0):q + 2])
    return bytes(y)


def pw_sweep():
    """(p, W): every anchor position of the sweep under every band of the sweep."""
    return [(p, W) for p in P_SWEEP for W in W_SWEEP]


def spread(n, lo, hi):
    """n positions in [lo, hi), at least 4 apart: isolated substitutions in random sequence cost 1 each, and no
    alignment with indels is cheaper."""
    assert (hi - lo) >= 4 * n
    return [lo + (k * (hi - lo)) // n for k in range(n)]


# ------------------------------------------------------------------------------------------------ substitutions
def subs_pair(seed, p, L, positions, tail=40):
    """a = U + X, b = X with substitutions at ``positions`` + 40 random bases (so lb > rem + 30: no B row)."""
    X = rnd(L, seed, 1)
    return [rnd(p, seed, 0) + X, with_subs(X, positions) + rnd(tail, seed, 2)]


def subs_cases(name, seed, p, L, positions, one_more, W):
    """``len(positions)`` isolated substitutions on the main diagonal: the A row ends at j = rem = L with cost
    E = len(positions) (a substitution on the last row ties with deleting x's last base, cell j = L - 1, and the main
    diagonal wins).  One substitution more (``one_more``) at the same E: cost E + 1, no row."""
    E = len(positions)
    yield (name + "_hit", subs_pair(seed, p, L, positions), M, E, W, [(0, 1, p, p + L, 0, L)])
    yield (name + "_miss", subs_pair(seed, p, L, sorted(positions + [one_more])), M, E, W, [])


def cost_threshold_cases():
    for k, (p, W) in enumerate(pw_sweep()):
        E = [1, 2, 3, 6, 12][k % 5]
        pos = spread(E + 1, 33, 118)
        yield from subs_cases("cost_p%d_W%d_E%d" % (p, W, E), 100 + k, p, 120, pos[:E], pos[E], W)


# ------------------------------------------------------------------------------------------------ band edge
def band_edge_cases():
    """One run of n inserted (or deleted) bases at x[40], then 140 clean bases.  n = W = E: the path shifts by W
    diagonals, stays inside the band and ends at j = L + W (L - W) with cost W.  n = W + 1 = E: the cost would fit, the
    shift does not; inside the band the last 109 or more bases face unrelated ones."""
    L = 180
    for k, (p, W) in enumerate(pw_sweep()):
        seed = 300 + k
        a = rnd(p, seed, 0) + rnd(L, seed, 1)
        X = a[p:]
        V = rnd(40, seed, 2)
        ins = rnd(W + 1, seed, 3)
        yield ("ins_p%d_W%d_hit" % (p, W), [a, X[:40] + ins[:W] + X[40:] + V], M, W, W, [(0, 1, p, p + L, 0, L + W)])
        yield ("ins_p%d_W%d_miss" % (p, W), [a, X[:40] + ins + X[40:] + V], M, W + 1, W, [])
        yield ("del_p%d_W%d_hit" % (p, W), [a, X[:40] + X[40 + W:] + V], M, W, W, [(0, 1, p, p + L, 0, L - W)])
        yield ("del_p%d_W%d_miss" % (p, W), [a, X[:40] + X[41 + W:] + V], M, W + 1, W, [])


# ------------------------------------------------------------------------------------------------ canA / canB
def can_edge_cases():
    L = 100
    for k, W in enumerate(W_SWEEP):
        for p in (5, 64):
            seed = 500 + 2 * k + (p == 64)
            a = rnd(p, seed, 0) + rnd(L, seed, 1)
            X = a[p:]
            V = rnd(W + 1, seed, 2)
            n = "_p%d_W%d" % (p, W)
            # b = the first L - W bases of x.  rem = lb + W: row rem has ONE cell inside the band with j <= lb, (rem, lb),
            # reached by deleting x's last W bases -> A ends at j = lb with cost W = E; b is also contained exactly: B ends
            # at i = lb with cost 0.  Both rows from one candidate.
            yield ("canA_on" + n, [a, X[:L - W]], M, W, W, [(0, 1, p, p + L, 0, L - W), (0, 1, p, p + L - W, 0, L - W)])
            # one base shorter: rem = lb + W + 1, no cell of row rem inside the band has j <= lb -> the B row only
            yield ("canA_off" + n, [a, X[:L - W - 1]], M, W + 1, W, [(0, 1, p, p + L - W - 1, 0, L - W - 1)])
            # b = x + W more bases.  lb = rem + W: column lb has ONE cell inside the band with i <= rem, (rem, lb), reached by
            # inserting b's last W bases -> B ends at i = rem with cost W = E; the A row ends at j = rem with cost 0.
            yield ("canB_on" + n, [a, X + V[:W]], M, W, W, [(0, 1, p, p + L, 0, L), (0, 1, p, p + L, 0, L + W)])
            # one base longer: lb = rem + W + 1 -> the A row only
            yield ("canB_off" + n, [a, X + V], M, W + 1, W, [(0, 1, p, p + L, 0, L)])


# ------------------------------------------------------------------------------------------------ phases of the row walk
def first_fast_row(p, W):
    """k_extend_bits walks rows one by one while i <= W + 1 or x[i - 1] is not the first base of a 32-bit word of a, then
    in blocks of 16 rows: the first row of the first block."""
    i = W + 2
    while (p + i - 1) % 16:
        i += 1
    return i


def phase_cases():
    """Substitutions on the rows where the bit-vector kernel changes phase (and wherever that puts them for the other two
    mappings): E = their number gives the main-diagonal row, one more substitution gives none (``subs_cases``)."""
    L = 200
    lane_bands = [1, 4, 5, 8, 9, 15]                       # (the bands of the two lane mappings, cycling under the positions)
    combos = [(p, lane_bands[k % 6]) for k, p in enumerate(P_SWEEP)] + [(64, 15), (16, 1), (7, 16), (7, 30)]
    for k, (p, W) in enumerate(combos):
        blk = first_fast_row(p, W)
        while blk < 33:                                    # a block start behind the anchor
            blk += 16
        r64 = blk
        while (p + r64 - 1) % 64:                          # first row of a 64-row round
            r64 += 16
        extra = 170                                        # (the one substitution more: a row of its own, away from the others)
        places = {
            "first": [33],                                 # the first row after the anchor
            "last": [L],                                   # the last row (ties with the deletion of x's last base)
            "blk": [blk + 14, blk + 15, blk + 16],         # rows 15, 16, 17 of a block of 16
            "r64": [r64 + 62, r64 + 63, r64 + 64],         # rows 63, 64, 65 of a round of 64
            "lim": [L - 2, L - 1],                         # the row before rem - 1, where the blocks end, and that row ("last": the one after)
        }
        for tag, rows in places.items():
            pos = [r - 1 for r in rows]
            assert extra not in pos and max(pos) < L
            yield from subs_cases("phase_%s_p%d_W%d" % (tag, p, W), 700 + k, p, L, pos, extra, W)
        # the same for a B row: b = X (200 bases) with substitutions on the rows before and after lb - W - 1, inside
        # a = U + X + 35 more bases (rem > lb + 30: no A row).  Cost 3 on the main diagonal at i = lb; the last W rows are clean.
        seed = 750 + k
        X = rnd(L, seed, 1)
        a = rnd(p, seed, 0) + X + rnd(35, seed, 2)
        pos = [L - W - 3, L - W - 2, L - W - 1]
        yield ("phase_limB_p%d_W%d_hit" % (p, W), [a, with_subs(X, pos)], M, 3, W, [(0, 1, p, p + L, 0, L)])
        yield ("phase_limB_p%d_W%d_miss" % (p, W), [a, with_subs(X, [100] + pos)], M, 3, W, [])


# ------------------------------------------------------------------------------------------------ early stop
def early_stop_cases():
    """All E substitutions close together, then a long clean remainder: the band minimum stands AT E when the kernels test
    it, and the row must still be reported; with E + 1 it must not (``subs_cases``)."""
    for k, p in enumerate(range(1, 17)):                   # inside the first 16 rows after the anchor, 210 clean rows behind
        W = W_SWEEP[k % len(W_SWEEP)]
        E = 1 + k % 3
        pos = [32, 37, 42, 47][:E + 1]
        yield from subs_cases("stop16_p%d_W%d_E%d" % (p, W, E), 900 + k, p, 258, pos[:E], pos[E], W)
    for k, p in enumerate([1, 2, 16, 62, 63, 64, 65]):     # around rows 64 and 128 (the 64-row rounds), 100 clean rows behind
        W = W_SWEEP[(k + 3) % len(W_SWEEP)]
        for r in (64, 128):
            yield from subs_cases("stop%d_p%d_W%d" % (r, p, W), 950 + k, p, 230, [r - 2, r - 1, r], r + 3, W)


# ------------------------------------------------------------------------------------------------ ties
def tie_cases():
    """Low-complexity ends: several cells of the end row (column) hold the smallest cost.  In every pair the cost is 1
    (E = 1); a substitution at x[35] more makes it 2: no row."""
    L = 60
    for k, W in enumerate([1, 4, 5, 8, 15, 16]):
        p = (3, 64)[k % 2]
        seed = 1100 + k
        U = rnd(p, seed, 0)
        X = rnd(L - 1, seed, 1) + b"G"
        V = rnd(40, seed, 2)
        V2 = rnd(50, seed, 3)
        n = "_p%d_W%d" % (p, W)

        def both(name, a, b, row):
            yield (name + n + "_hit", [a, b], M, 1, W, [row])
            yield (name + n + "_miss", [a, with_subs(b, [35])], M, 1, W, [])

        # a ends in A x 12; b lacks X's last base (G) and goes on with A x 20.  G -> A on the main diagonal costs 1 and ends at
        # j = rem; deleting G costs 1 and ends at j = rem - 1.  Closest to the main diagonal: j = rem.
        rem = L + 12
        yield from both("tieA_homopolymer", U + X + b"A" * 12, X[:-1] + b"A" * 20 + V, (0, 1, p, p + rem, 0, rem))
        # a ends in (AC) x 6; b has one C more in front of its (AC) x 10.  Inserting that C (j = rem + 1) and deleting the
        # array's first A (j = rem - 1) both cost 1, the main diagonal needs both (2): equally close, the smaller j wins.
        yield from both("tieA_AC", U + X + b"AC" * 6, X + b"C" + b"AC" * 10 + V, (0, 1, p, p + rem, 0, rem - 1))
        # the mirror for B rows: b = X without its last base + A x 12, inside a = U + X + A x 20 + 50 more.  G -> A ends at
        # i = lb, deleting G at i = lb + 1, both cost 1: i = lb.
        lb = L - 1 + 12
        yield from both("tieB_homopolymer", U + X + b"A" * 20 + V2, X[:-1] + b"A" * 12, (0, 1, p, p + lb, 0, lb))
        # b = X + C + (AC) x 6 inside a = U + X + (AC) x 10 + 50 more: i = lb - 1 (insert the C) and i = lb + 1 (delete the
        # array's first A) cost 1, i = lb costs 2: the smaller i wins.
        lb = L + 13
        yield from both("tieB_AC", U + X + b"AC" * 10 + V2, X + b"C" + b"AC" * 6, (0, 1, p, p + lb - 1, 0, lb))


# ------------------------------------------------------------------------------------------------ two anchors, no self-repeat
def two_anchor_pair(unit, n, zlen):
    """a = U + unit x (n + 1) + Z', b = unit x n + Z' + 20 more: b's 32-base prefix stands in a at p = len(U) and one
    unit later, and nowhere in b again (Z' starts with T)."""
    assert len(unit) * n >= 32
    U = rnd(39, 1300, len(unit)) + b"G"
    Z = b"T" + rnd(zlen - 1, 1301, len(unit))
    return [U + unit * (n + 1) + Z, unit * n + Z + rnd(20, 1302, len(unit))]


def two_anchor_cases(long=False):
    """Two anchors of one pair that both reach a's end.  From the second (p + |unit|) b matches a's tail exactly: cost 0,
    j = rem.  From the first a has one unit more than b: deleting it costs |unit| and needs a band of |unit|, the A row then
    ends |unit| columns left of the diagonal -- the same bend.  Longest only: the row of the first anchor where E and W
    reach it, else the row of the second.  lb = rem(p) + 17 or more: B rows only where the band is 17 or wider -- never.
    ``long``: tails of 40 bases and min_length 64, so that both indexes take the pair."""
    zlen, m = (40, 64) if long else (30, 40)
    tag = "_long" if long else ""
    seqs = two_anchor_pair(b"AC", 16, zlen)                       # |a| = 40 + 34 + zlen, p = 40 and 42
    la, bend = 74 + zlen, 32 + zlen
    for E, W, p in ((2, 2, 40), (3, 5, 40), (2, 1, 42), (1, 2, 42)):
        yield ("two_anchors_AC%s_E%d_W%d" % (tag, E, W), seqs, m, E, W, [(0, 1, p, la, 0, bend)])
    seqs = two_anchor_pair(b"ACG", 11, zlen)                      # prefix K-mer = (ACG) x 10 + AC; p = 40 and 43
    la, bend = 76 + zlen, 33 + zlen
    for E, W, p in ((3, 3, 40), (4, 6, 40), (3, 2, 43), (2, 3, 43)):
        yield ("two_anchors_ACG%s_E%d_W%d" % (tag, E, W), seqs, m, E, W, [(0, 1, p, la, 0, bend)])


# ------------------------------------------------------------------------------------------------ selection overflow
OVERFLOW_M, OVERFLOW_E, OVERFLOW_W = 64, 3, 2


def overflow_case():
    """One read whose candidate list holds more than 256 accepted A candidates (the LDS table of the longest-only selection
    takes 256), with a non-self-repeating b of two accepted anchors in the SAME list.

    a = R30 + (AC) x 120 + GT (272 bases).  b1..b4 = (AC) x 125 + 10 random bases: their prefix stands at every even
    p = 30 .. 208 of a (90 anchors each), and from each of them a's tail differs from b by its last two bases only (GT
    against AC): cost 2 <= E, 360 accepted A candidates, ONE A row per b: the longest, p = 30, ending on the main diagonal
    at j = rem = 242.
    b5 = (AC) x 16 + AG + (AC) x 14 + GT + 50 random bases does not repeat its prefix (AG follows it).  From p = 208
    (rem 64) a's tail is b5's first 64 bases but for AG against AC: cost 1.  From p = 206 there is one AC more: cost 3 with a
    band of 2; from p = 204 two more: out of reach.  Its A row: p = 206, j = 64 (two columns left of the diagonal).
    No B rows: every b is longer than rem + W everywhere.  b1..b4 among themselves differ in their 10-base tails behind
    250 bases of AC: more than 3 differences at every anchor that reaches an end."""
    a = rnd(29, 1400, 0) + b"G" + b"AC" * 120 + b"GT"
    seqs = [a] + [b"AC" * 125 + rnd(10, 1400, i) for i in range(1, 5)]
    seqs.append(b"AC" * 16 + b"AG" + b"AC" * 14 + b"GT" + rnd(50, 1400, 5))
    expect = [(0, i, 30, 272, 0, 242) for i in range(1, 5)] + [(0, 5, 206, 272, 0, 64)]
    return ("select_overflow", seqs, OVERFLOW_M, OVERFLOW_E, OVERFLOW_W, expect)


def overflow_preconditions(case, extend_pairs):
    """What makes the overflow case reach the global (a, b) table, from the restatement's DP (``extend_pairs`` =
    oracle.extend_oracle.extend_pairs) on every candidate of read 0's list: (accepted A candidates in the list, accepted
    anchors of read 5).  Read 5 must not repeat its own prefix K-mer."""
    _, seqs, m, max_diff, band, _ = case
    a, b5 = seqs[0], seqs[5]
    assert b5.find(b5[:32], 1) == -1
    cat = np.frombuffer(b"".join(seqs) + b"\0" * 64, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    cand = [(p, b) for b in range(1, len(seqs)) for p in range(len(a) - m + 1) if a[p:p + 32] == seqs[b][:32]]
    res = extend_pairs(cat, np.array([offs[0] + p for p, _ in cand], dtype=np.uint64), np.array([len(a) - p for p, _ in cand], dtype=np.uint32),
                       np.array([offs[b] for _, b in cand], dtype=np.uint64), np.array([len(seqs[b]) for _, b in cand], dtype=np.uint32),
                       max_diff, band)
    ok_a = np.asarray(res)[:, 0] == 1
    return int(ok_a.sum()), sorted(p for (p, b), ok in zip(cand, ok_a) if ok and b == 5)


# ------------------------------------------------------------------------------------------------ generated sets
def mutate(rng, s, n):
    r = bytearray(s)
    for _ in range(n):
        q = int(rng.integers(0, len(r)))
        kind = int(rng.integers(3))
        if kind == 0:
            r[q] = b"ACGT"[int(rng.integers(4))]
        elif kind == 1 and len(r) > 8:
            del r[q]
        else:
            r.insert(q, b"ACGT"[int(rng.integers(4))])
    return bytes(r)


def band_sweep_case(W, eight_bit=False):
    """One small set per band: six reads of a 500-base random genome (60-300 bases) and six of period-1, 2, 3 and 5 tandem
    arrays (60-140 bases), sparse substitutions and indels, every other read reverse-complemented.  ``eight_bit``: the same
    reads with N and lower-case bytes in three of them, 24 in the first -- dense enough that the library stores 8 bits per
    base (anchor K = 8)."""
    rng = np.random.default_rng(5000 + W)
    genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=500))
    units = [b"A", b"AC", b"ACG", b"ACGTT"]
    reads = []
    for k in range(12):
        if k % 2 == 0:
            ln = int(rng.integers(60, 301))
            st = int(rng.integers(0, len(genome) - ln + 1))
            r = genome[st:st + ln]
        else:
            u = units[(k // 2 + W) % 4]
            ln = int(rng.integers(60, 141))
            ph = int(rng.integers(0, len(u)))
            r = (u * (ln // len(u) + 2))[ph:ph + ln]
        r = mutate(rng, r, int(rng.integers(0, 4)))[:300]
        reads.append(r.translate(RC)[::-1] if k % 4 >= 2 else r)
    max_diff = max(1, [1, W, 40][W % 3])
    m = [12, 40, 64][(W // 3) % 3]
    if eight_bit:
        for k, n_bad in ((0, 24), (5, 3), (8, 2)):
            r = bytearray(reads[k])
            for q in rng.choice(len(r), size=n_bad, replace=False):
                r[q] = ord("N") if q % 3 == 0 else ord(chr(r[q]).lower())
            reads[k] = bytes(r)
    return ("band_sweep%s_W%d" % ("_8bit" if eight_bit else "", W), reads, m, max_diff, W, None)


def fuzz_case(t):
    """Seeded set t: a random, a period-1..3 tandem or a two-letter genome; 3-8 reads of 20-160 bases with up to three
    edits each, some reverse-complemented; W from 0..30, E from {1, 2, 3, 6, 12}, min_length from {8, 12, 20, 33}."""
    rng = np.random.default_rng(9000 + t)
    kind = t % 3
    if kind == 0:
        genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=300))
    elif kind == 1:
        u = [b"A", b"AC", b"ACG"][int(rng.integers(3))]
        genome = u * (300 // len(u))
    else:
        genome = bytes(b"AC"[i] for i in rng.integers(0, 2, size=300))
    reads = []
    for _ in range(int(rng.integers(3, 9))):
        ln = int(rng.integers(20, 161))
        st = int(rng.integers(0, len(genome) - ln + 1))
        r = mutate(rng, genome[st:st + ln], int(rng.integers(0, 4)))
        reads.append(r.translate(RC)[::-1] if rng.random() < 0.25 else r)
    W = int(rng.integers(0, 31))
    E = int(rng.choice([1, 2, 3, 6, 12]))
    m = int(rng.choice([8, 12, 20, 33]))
    return ("fuzz%d" % t, reads, m, E, W, None)


# ------------------------------------------------------------------------------------------------ the families
FAMILIES = {
    "cost_threshold": cost_threshold_cases,
    "band_edge": band_edge_cases,
    "can_edges": can_edge_cases,
    "phases": phase_cases,
    "early_stop": early_stop_cases,
    "ties": tie_cases,
    "two_anchors": two_anchor_cases,
}


def constructed_cases(family):
    return list(FAMILIES[family]())
