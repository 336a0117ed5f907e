"""TEST INFRASTRUCTURE ONLY -- the inexact extension mode (``po_overlaps_ex``) stated a second time, independently.

The reference overlapper is exact, so nothing of it can check ``max_diff > 0``.  ``oracle/extend_oracle.c`` is the
build's restatement of the mode and the checker of every GPU test; THIS file is what that restatement is held
against (tests/test_extend_definition.py).  It is written from the *Definition* paragraph at the top of
oracle/extend_oracle.c and phasm_amd/csrc/extend.hip.h, not from their code, and differs from both in every choice
a second writer is free to make:

* the FULL ``(rem + 1) x (lb + 1)`` matrix is kept, the band is a mask laid over it (no band-relative indexing);
* the horizontal dependency of a row is a running minimum (``D[i][j] = j + min_k<=j (t[k] - k)``), no left-to-right
  loop over cells;
* the end cell is the minimum of plain tuples ``(cost, |j - i|, coordinate)`` -- "closest to the main diagonal,
  then the smaller coordinate" as the header says it -- not a packed integer key;
* anchors, the longest-only rule for A rows and the every-occurrence rule for B rows are loops over Python bytes.

Plain numpy, nothing compiled, no ctypes.  Meant for reads of a few hundred bases.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

INF = 1 << 40


def _as_bytes(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def mismatches(x: bytes, y: bytes) -> np.ndarray:
    """``neq[i][j] = 1`` where ``x[i] != y[j]``, else 0."""
    return (np.frombuffer(x, dtype=np.uint8)[:, None] != np.frombuffer(y, dtype=np.uint8)[None, :]).astype(np.int64)


def band_matrix(x: bytes, y: bytes, W: int, neq: Optional[np.ndarray] = None) -> np.ndarray:
    """``D[i][j]`` = unit-cost edit distance of ``x[:i]`` and ``y[:j]`` over paths that stay inside ``|j - i| <= W``;
    cells outside the band hold ``INF``.  ``neq[i][j] = x[i] != y[j]`` may be passed in (a slice of a larger one)."""
    n, l = len(x), len(y)
    if neq is None:
        neq = mismatches(x, y)
    jj = np.arange(l + 1, dtype=np.int64)
    # the band as a mask over the whole matrix: INF added to every cell outside it (and the sum cut back to INF)
    mask = np.where(np.abs(jj[None, :] - np.arange(n + 1, dtype=np.int64)[:, None]) > W, INF, 0)
    D = np.empty((n + 1, l + 1), dtype=np.int64)
    np.minimum(jj + mask[0], INF, out=D[0])
    t = np.empty(l + 1, dtype=np.int64)
    for i in range(1, n + 1):
        prev = D[i - 1]
        t[0] = prev[0] + 1                                            # only from above
        np.minimum(prev[:-1] + neq[i - 1], prev[1:] + 1, out=t[1:])   # diagonal step, step down
        t += mask[i]
        row = np.minimum.accumulate(t - jj) + jj                      # ... then any number of steps to the right
        row += mask[i]
        np.minimum(row, INF, out=D[i])
    return D


def extend(x: bytes, y: bytes, E: int, W: int, neq: Optional[np.ndarray] = None) -> Tuple[Optional[int], Optional[int]]:
    """One candidate: ``(j*, i*)`` -- the end column of the A row and the end row of the B row, ``None`` where the
    candidate gives no such row."""
    rem, lb = len(x), len(y)
    D = band_matrix(x, y, W, neq)
    jA = iB = None
    if rem <= lb + W:
        ends = [(int(D[rem][j]), abs(j - rem), j) for j in range(1, lb + 1) if D[rem][j] <= E]
        if ends:
            jA = min(ends)[2]
    if lb <= rem + W:
        ends = [(int(D[i][lb]), abs(lb - i), i) for i in range(1, rem + 1) if D[i][lb] <= E]
        if ends:
            iB = min(ends)[2]
    return jA, iB


def candidates(seqs: Sequence[bytes], m: int, K: int) -> List[Tuple[int, int, int]]:
    """Every anchor ``(a, p, b)``: b's K-byte prefix stands at ``a[p:p + K]``, ``p <= la - m``, both reads at least
    ``m`` long, a and b different reads."""
    out = []
    for a, sa in enumerate(seqs):
        if len(sa) < m:
            continue
        for b, sb in enumerate(seqs):
            if b == a or len(sb) < m:
                continue
            head = sb[:K]
            p = sa.find(head)
            while p != -1 and p <= len(sa) - m:
                out.append((a, p, b))
                p = sa.find(head, p + 1)
    return out


def overlaps_ex(seqs: Sequence, min_length: int, max_diff: int, band: int, anchor: int = 32) -> np.ndarray:
    """Sorted (n, 6) int64 rows ``(a, b, astart, aend, 0, bend)`` of the extension mode."""
    seqs = [_as_bytes(s) for s in seqs]
    m = max(int(min_length), 1)
    K = min(int(anchor), m)
    E = int(max_diff)
    W = int(band) if E else 0
    rows = []
    longest = {}          # (a, b) -> (smallest accepted p, its row)
    neq_of = {}
    for a, p, b in candidates(seqs, m, K):
        if (a, b) not in neq_of:
            neq_of = {(a, b): mismatches(seqs[a], seqs[b])}      # (one pair's matrix at a time: candidates come pair by pair)
        jA, iB = extend(seqs[a][p:], seqs[b], E, W, neq_of[(a, b)][p:])
        la, lb = len(seqs[a]), len(seqs[b])
        if jA is not None and ((a, b) not in longest or p < longest[(a, b)][0]):
            longest[(a, b)] = (p, (a, b, p, la, 0, jA))
        if iB is not None:
            rows.append((a, b, p, p + iB, 0, lb))
    rows += [r for _, r in longest.values()]
    out = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    if len(out):
        out = out[np.lexsort(out.T[::-1])]
    return out
