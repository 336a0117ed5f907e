"""The hot loop of `phasm phase` on the device: scoring and pruning the haplotype extensions at one bubble.

What the reference's ``BubbleChainPhaser.branch`` (``generate_new_hsets`` + ``calculate_rl``, phasm/phasing.py:421-480, 564-631),
``prune`` (phasing.py:482-539) and the per-path score of ``phase_large_bubble`` (phasing.py:633-685) compute, through
``po_phase_branch`` (include/phasm_overlap.h):

    bubble = pack_bubble(possible_paths, [hs.read_sets for hs in candidate_sets], relevant_reads)
    cand, ext, rl = branch(ov, bubble, start_of_block, threshold, min_spanning_reads)
    cand, ext, rl = branch_and_prune(ov, bubble, start_of_block, threshold, min_spanning_reads,
                                     prune_factor, prune_step_size, max_candidates, max_prune_rounds)
    scores = score_paths(ov, bubble)

Entry j of the result is candidate set ``cand[j]`` extended by the paths ``ext_digits(ext[j], P, k)``, with relative likelihood
``rl[j]`` (log10), in the order of the list the reference returns.

``ov`` is a SCORER: anything with ``phase_branch(bubble, start_of_block, min_spanning_reads, threshold, levels,
max_candidates, want_table)`` and ``phase_stats()`` -- an ``ExactOverlapper`` (the device) or a ``HostScorer`` (the same
decomposition in numpy, for machines without a GPU and for the tests; it is no fallback: nothing here picks it on its own).

What feeds that call -- the reference's ``read_alignments`` mapping (phasm/cli/assembler.py:313-328), ``get_aligning_reads``
(phasing.py:541-550), the spanning-read intersection (phasing.py:263-286) and ``get_relevant_read_info`` (phasing.py:366-419) --
through ``po_phase_index`` and ``po_phase_relevant``, on oriented read ids:

    index = ov.phase_index(rows)                                                     # once
    rel = relevant_reads(ov, index, cur_graph, prev_graph, prev_aligning, preds, start_of_block, min_spanning_reads)
    bubble = bubble_from_relevant(rel, ploidy, paths, read_sets)                     # then branch(...) as above

Here ``ov`` is anything with ``phase_relevant``: an ``ExactOverlapper`` or a ``HostIndex`` (numpy, like ``HostScorer``).

What ``phase()`` computes per bubble before any of that (phasing.py:196-234, 396) -- the order of the bubbles along their chain,
``networkx.all_simple_paths(g, entrance, exit)``, ``superbubble_nodes(g, entrance, exit) - {entrance, exit}`` and the
predecessors of the exit with their edge weights -- for every top-level bubble of a graph in one call, through
``po_phase_paths``:

    paths = bubble_paths(ov, graph_res, max_paths)                                   # once per graph: a BubblePaths
    for b in paths.chain_bubbles(chain):                                             # the order of phase()'s walk
        if paths.is_large(b, max_bubble_size): ...                                   # from the count alone
        paths.paths_of(b), paths.interior_of(b), paths.preds_of(b)

Here ``ov`` is anything with ``phase_paths``: an ``ExactOverlapper`` or a ``HostPaths`` (plain Python, like ``HostScorer``).

The walk loop of ``phase()`` itself, ``new_block`` and the final ``prune(.., 1.0)`` (phasing.py:182-364), with the candidate sets
resident on the device from bubble to bubble, through ``po_walk_*``:

    walk = ov.phase_walk(ploidy)                                                     # a DeviceWalk; HostWalk(scorer, ploidy) in numpy
    for block in phase_chain(ov, ov, index, chain_bubbles_input(paths, chain, reads_of_node), reads_of_node, ploidy, walk=walk):
        block.haplotypes, block.read_sets, block.include_last, block.from_large_bubble, block.log_rl, block.tie

One turn of that loop without the host between the gather and the step -- ``prev_graph_reads`` / ``prev_aligning_reads`` as
bitsets of the walk, the relevant arrays and the block-stable read ids on the device -- through ``po_walk_relevant`` and
``po_walk_step_resident``; ``phase_chain(..., resident=True)`` walks by it:

    rel = walk.relevant(ov, index, cur_graph, preds, start_of_block, min_spanning_reads)   # the six sizes; fetch() for the arrays
    cand, ext, rl = walk.step_resident(rel, path_reads, start_of_block, threshold, min_spanning_reads, levels, max_candidates)
    prev_graph, prev_aligning = walk.prev_sets()

The large arm of that walk for a bubble of ANY listed size (``phase_large_bubble``, phasing.py:633-685), with the paths
RESIDENT on the device, through ``po_phase_large``: the score of a path decomposes over its interior
nodes, so an interval per (interior node, read) suffices and every listed path is scored where ``po_phase_paths`` left it:

    paths = ov.phase_paths_resident(graph_res, max_listed_paths)                     # a DevicePaths; close() it
    bubbles = chain_bubbles_input(paths, chain, reads_of_node, resident_above=64)    # larger bubbles: "paths": None, "scorer"
    best, best_scores, scores = paths.score_large(b, rel, reads_of_node, n_best)     # what phase_chain calls at such a bubble
    paths.path_of(b, best[0])                                                        # the winner's node tuple alone

``HostResidentPaths(bubble_paths)`` is the same interface in numpy over a fully listed ``BubblePaths`` (the same
decomposition and tie rule; its summation order may differ from the device's).  Like ``HostScorer`` it is no fallback.

Not here: ``CoverageModel`` (unused by the reference), the debug data log, per-read probabilities."""
from __future__ import annotations

import math
import random
from collections import namedtuple
from dataclasses import dataclass, field, replace
from typing import Callable, Iterable, List, Optional, Sequence

import numpy as np

from ._lib import BUBBLE_PATHS_DTYPE, PATHS_BARE, PATHS_MANY, PATHS_SATURATED, PATHS_UNLISTED

NO_START = 0x7FFFFFFF


@dataclass
class PackedBubble:
    """One bubble as ``po_phase_branch`` takes it: local read ids 0..n_b-1 and CSR arrays (include/phasm_overlap.h)."""
    ploidy: int
    n_paths: int
    n_cands: int
    n_reads: int
    n_b: int
    overlap_max: np.ndarray      # int32 [R]
    aln_off: np.ndarray          # uint32 [R + 1]
    aln_b: np.ndarray            # uint32
    aln_a0: np.ndarray           # int32
    aln_a1: np.ndarray           # int32
    path_off: np.ndarray         # uint32 [P + 1]
    path_ids: np.ndarray         # uint32
    set_off: np.ndarray          # uint32 [C * k + 1]
    set_ids: np.ndarray          # uint32
    b_reads: list = field(default_factory=list)   # local id -> the caller's read object (empty when packed from arrays)

    def path_reads(self, p: int) -> np.ndarray:
        return self.path_ids[self.path_off[p]:self.path_off[p + 1]]

    def set_reads(self, c: int, i: int) -> np.ndarray:
        s = c * self.ploidy + i
        return self.set_ids[self.set_off[s]:self.set_off[s + 1]]


def _csr(lists: Sequence[Sequence[int]], dtype=np.uint32):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    if len(lists):
        off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.asarray([v for x in lists for v in x], dtype=dtype)
    return off, np.ascontiguousarray(flat)


def bubble_from_arrays(ploidy: int, overlap_max, alignments, paths, read_sets, n_b: Optional[int] = None) -> PackedBubble:
    """A bubble from local ids: ``alignments[r]`` the (b, arange0, arange1) triples of read r, ``paths[p]`` the interior ids of
    path p, ``read_sets[c][i]`` the ids of slot i of candidate c."""
    alignments = [list(a) for a in alignments]
    aln_off, aln_b = _csr([[t[0] for t in a] for a in alignments])
    _, a0 = _csr([[t[1] for t in a] for a in alignments], np.int32)
    _, a1 = _csr([[t[2] for t in a] for a in alignments], np.int32)
    path_off, path_ids = _csr([sorted(set(p)) for p in paths])
    flat_sets = [sorted(set(s)) for c in read_sets for s in c]
    if any(len(c) != ploidy for c in read_sets):
        raise ValueError("every candidate needs one read set per haplotype")
    set_off, set_ids = _csr(flat_sets)
    if n_b is None:
        n_b = int(max([-1] + aln_b.tolist() + path_ids.tolist() + set_ids.tolist())) + 1
    return PackedBubble(int(ploidy), len(paths), len(read_sets), len(alignments), int(n_b),
                        np.ascontiguousarray(np.asarray(overlap_max, dtype=np.int64).astype(np.int32)), aln_off, aln_b, a0, a1,
                        path_off, path_ids, set_off, set_ids)


def _default_expand(node) -> Iterable:
    """``get_all_reads`` of one node (phasing.py:552-562): the reads of a merged node, else the node itself."""
    reads = getattr(node, "reads", None)
    return reads if reads is not None else (node,)


def _triple(la):
    if hasattr(la, "arange"):
        return la.get_oriented_reads()[1], int(la.arange[0]), int(la.arange[1])
    b, a0, a1 = la
    return b, int(a0), int(a1)


def pack_bubble(paths, cand_read_sets, relevant, expand: Optional[Callable] = None) -> PackedBubble:
    """Objects to local ids and CSR arrays.  ``paths``: the possible paths through the bubble, each a tuple of nodes WITH its
    entrance and exit (they are left out here, as ``hap_ext[1:-1]``); ``expand(node)`` yields the reads of a node (default:
    ``node.reads`` where there is one, else the node).  ``cand_read_sets[c][i]``: ``read_sets[i]`` of candidate set c.
    ``relevant``: read -> (alignments, overlap_max), alignments being (b, arange0, arange1) triples or objects with ``.arange``
    and ``.get_oriented_reads()``.  Objects need ``__hash__`` and ``__eq__`` only.  The local id of a read is its place in the
    order in which the alignments first name it as b read; reads that no alignment names can never match and are dropped."""
    expand = expand or _default_expand
    local = {}
    overlap_max, alignments = [], []
    for _read, info in relevant.items():
        las, om = info[0], info[1]
        mine = []
        for la in las:
            b, a0, a1 = _triple(la)
            mine.append((local.setdefault(b, len(local)), a0, a1))
        alignments.append(mine)
        overlap_max.append(int(om))
    ids = lambda reads: [local[r] for r in reads if r in local]   # noqa: E731
    path_lists = [ids(r for node in tuple(p)[1:-1] for r in expand(node)) for p in paths]
    cand_read_sets = [list(c) for c in cand_read_sets]
    if not cand_read_sets:
        raise ValueError("there must be at least one candidate set")
    ploidy = len(cand_read_sets[0])
    out = bubble_from_arrays(ploidy, overlap_max, alignments, path_lists, [[ids(s) for s in c] for c in cand_read_sets], len(local))
    out.b_reads = list(local)
    return out


def ext_digits(ext: int, n_paths: int, ploidy: int) -> tuple:
    """The path index of every haplotype slot of extension id ``ext``: digits base P, slot 0 most significant."""
    out = []
    for _ in range(ploidy):
        out.append(int(ext) % n_paths)
        ext = int(ext) // n_paths
    return tuple(reversed(out))


def prune_levels(prune_factor: float, step: float, max_rounds: int) -> List[float]:
    """log10 of the prune factors the reference's loop can reach, in its order (phasing.py:496-521): the factor itself, then
    ``factor += step`` in float while fewer than ``max_rounds`` rounds have run and the factor is below 1.0.  A factor <= 0
    gives no level (``prune`` returns its input).  Whether the loop GOES on to a level also depends on how many candidates the
    level before left -- that is decided where the counts are."""
    if prune_factor <= 0.0:
        return []
    levels = [math.log10(prune_factor)]
    rounds = 1
    while rounds < max_rounds and prune_factor < 1.0:
        prune_factor += step
        levels.append(math.log10(prune_factor))
        rounds += 1
    return levels


def log_threshold(threshold: float) -> float:
    return -math.inf if threshold == 0.0 else math.log10(threshold)


def branch(ov, bubble: PackedBubble, start_of_block: bool, threshold: float = 0.0, min_spanning_reads: int = 0):
    """The kept extensions of every candidate set, as ``BubbleChainPhaser.branch`` lists them: ``(cand, ext, rl)``."""
    return ov.phase_branch(bubble, start_of_block, min_spanning_reads, threshold)


def branch_and_prune(ov, bubble: PackedBubble, start_of_block: bool, threshold: float = 0.0, min_spanning_reads: int = 0,
                     prune_factor: float = 0.1, prune_step_size: float = 0.1, max_candidates: int = 500, max_prune_rounds: int = 9):
    """``prune(branch(...), prune_factor)`` of the reference: the survivors ``(cand, ext, rl)`` in the order of the kept list.
    ``prune_factor`` is a number (a callable of the reference's depends on the length of the kept list: call ``branch``, then
    this with the number)."""
    levels = prune_levels(float(prune_factor), float(prune_step_size), int(max_prune_rounds))
    return ov.phase_branch(bubble, start_of_block, min_spanning_reads, threshold, levels=levels, max_candidates=int(max_candidates))


def score_paths(ov, bubble: PackedBubble) -> np.ndarray:
    """The score of every path as ``phase_large_bubble`` computes it: the sum over the relevant reads of the overlap with the
    path's interior alone, divided by their number."""
    if bubble.n_reads == 0:
        raise ZeroDivisionError("no relevant reads")
    alone = replace(bubble, ploidy=1, n_cands=1, set_off=np.zeros(2, dtype=np.uint32), set_ids=np.zeros(0, dtype=np.uint32))
    *_, table = ov.phase_branch(alone, False, 0, 0.0, want_table=True, cap=0)
    return table.reshape(bubble.n_paths) / bubble.n_reads


def best_paths(scores: np.ndarray, ploidy: int) -> List[int]:
    """``sorted(scored_paths, key=scored_paths.get, reverse=True)[:ploidy]`` on path indices (a stable sort: ties keep the
    order of the paths)."""
    return sorted(range(len(scores)), key=lambda p: scores[p], reverse=True)[:ploidy]


class HostScorer:
    """The scheme of ``po_phase_branch`` in numpy: the table S[c][i][p], then every extension from it.  The same contract as
    the device's, up to the order of the float64 sums."""

    def __init__(self):
        self._stats = {}

    def phase_stats(self) -> dict:
        return dict(self._stats)

    @staticmethod
    def _intervals(b: PackedBubble, off, ids, n_sets):
        R, A = b.n_reads, len(b.aln_b)
        member = np.zeros((n_sets, max(b.n_b, 1)), dtype=bool)
        for s in range(n_sets):
            member[s, ids[off[s]:off[s + 1]]] = True
        s0 = np.full((n_sets, R), NO_START, dtype=np.int64)
        e = np.zeros((n_sets, R), dtype=np.int64)
        if A == 0 or R == 0:
            return s0, e
        read_of = np.repeat(np.arange(R), np.diff(b.aln_off.astype(np.int64)))
        match = member[:, b.aln_b]                                                  # [set, alignment]
        lo = np.where(match, b.aln_a0.astype(np.int64)[None, :], NO_START)
        hi = np.where(match, np.minimum(b.aln_a1.astype(np.int64), b.overlap_max.astype(np.int64)[read_of])[None, :], 0)
        some = np.flatnonzero(np.diff(b.aln_off.astype(np.int64)) > 0)
        starts = b.aln_off.astype(np.int64)[some]
        s0[:, some] = np.minimum.reduceat(lo, starts, axis=1)
        e[:, some] = np.maximum(np.maximum.reduceat(hi, starts, axis=1), 0)
        return s0, e

    def table(self, b: PackedBubble) -> np.ndarray:
        C, k, P, R = b.n_cands, b.ploidy, b.n_paths, b.n_reads
        ss0, se = self._intervals(b, b.set_off, b.set_ids, C * k)
        ps0, pe = self._intervals(b, b.path_off, b.path_ids, P)
        s0 = np.minimum(ss0[:, None, :], ps0[None, :, :])
        e = np.maximum(se[:, None, :], pe[None, :, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(s0 < e, (e - s0) / b.overlap_max.astype(np.float64)[None, None, :], 0.0)
        return f.sum(axis=2).reshape(C, k, P)

    def phase_branch(self, bubble: PackedBubble, start_of_block, min_spanning_reads: int = 0, threshold: float = 0.0, levels=None,
                     max_candidates: int = 0, cap: Optional[int] = None, want_table: bool = False):
        b = bubble
        C, k, P, R = b.n_cands, b.ploidy, b.n_paths, b.n_reads
        if not 1 <= k <= 8 or not 1 <= P <= 64 or C < 1 or C * P ** k >= 2 ** 31:
            raise ValueError("po_phase_branch: bad sizes")
        S = self.table(b)
        Pk = P ** k
        digits = np.stack(np.unravel_index(np.arange(Pk), (P,) * k), axis=1)       # [ext, slot], slot 0 most significant
        tot = np.zeros((C, Pk))
        for i in range(k):
            tot = tot + S[:, i, digits[:, i]]
        den = np.ones(Pk, dtype=np.int64)
        for i in range(k):
            same = np.ones(Pk, dtype=np.int64)
            for j in range(i):
                same += digits[:, j] == digits[:, i]
            den *= same
        with np.errstate(divide="ignore", invalid="ignore"):
            tot = tot / float(k * R) if R else np.zeros_like(tot)
            p_sr = np.where(tot == 0.0, -np.inf, np.log10(tot))
            prior = np.log10((math.factorial(k) // den).astype(np.float64) / float(Pk))
        rl = p_sr + prior[None, :]
        if R < min_spanning_reads:
            rl = np.full_like(rl, -np.inf)
        listed = np.ones(Pk, dtype=bool)
        if start_of_block:
            listed = np.all(digits[:, 1:] >= digits[:, :-1], axis=1)
        keep = (rl >= log_threshold(threshold)) & listed[None, :]
        cand, ext = np.nonzero(keep)
        rls = rl[cand, ext]
        st = {"n_extensions": int(C * listed.sum()), "n_kept": len(rls), "n_survivors": len(rls), "level_used": -1,
              "max_rl": float(rls.max()) if len(rls) else math.nan, "level_counts": [], "n_levels": len(levels) if levels is not None else 0}
        if levels is not None and len(levels) and len(rls) >= 2 and rls.max() != -np.inf:
            with np.errstate(invalid="ignore"):
                d = rls - rls.max()
            alive = np.ones(len(rls), dtype=bool)
            for j, level in enumerate(levels):
                alive &= d >= level
                st["level_counts"].append(int(alive.sum()))
                st["level_used"] = j
                if alive.sum() <= max_candidates:
                    break
            # (the counts of the levels the loop did not reach, as if it had)
            rest = alive.copy()
            for level in levels[st["level_used"] + 1:]:
                rest &= d >= level
                st["level_counts"].append(int(rest.sum()))
            cand, ext, rls = cand[alive], ext[alive], rls[alive]
            st["n_survivors"] = len(rls)
        st["level_counts"] = (st["level_counts"] + [0] * 16)[:16]
        self._stats = st
        n = len(rls) if cap is None else min(int(cap), len(rls))
        out = (cand[:n].astype(np.uint32), ext[:n].astype(np.uint32), rls[:n].astype(np.float64))
        return out + (S.reshape(-1).copy(),) if want_table else out


# ---- the relevant reads of a bubble (po_phase_index, po_phase_relevant) -------------------------------------------------------

ALIGNMENT_DTYPE = np.dtype([("b", np.uint32), ("a0", np.int32), ("a1", np.int32), ("seq", np.uint32)])


@dataclass
class RelevantReads:
    """What ``po_phase_relevant`` gives for one bubble.  ``overlap_max`` .. ``aln_a1`` are those fields of ``PackedBubble``;
    the local id of a read is its place in ``b_reads`` (ascending global ids)."""
    cur_aligning: np.ndarray     # uint32, ascending
    rel_reads: np.ndarray        # uint32 [R], ascending
    overlap_max: np.ndarray      # int32 [R]
    aln_off: np.ndarray          # uint32 [R + 1]
    aln_b: np.ndarray            # uint32, local ids
    aln_a0: np.ndarray           # int32
    aln_a1: np.ndarray           # int32
    b_reads: np.ndarray          # uint32 [n_b], ascending
    n_spanning: int = 0
    fell_back: bool = False

    def alignments_of(self, r: int) -> list:
        """The (global b read, a0, a1) triples of relevant read number ``r``."""
        lo, hi = int(self.aln_off[r]), int(self.aln_off[r + 1])
        return [(int(self.b_reads[b]), int(a0), int(a1)) for b, a0, a1 in zip(self.aln_b[lo:hi], self.aln_a0[lo:hi], self.aln_a1[lo:hi])]


def relevant_reads(src, index, cur_graph, prev_graph=(), prev_aligning=(), preds=(), start_of_block: bool = False,
                   min_spanning_reads: int = 0) -> RelevantReads:
    """The relevant reads of one bubble as ``phase()`` collects them: all aligning reads at the start of a block, else the
    spanning ones -- and if those are fewer than ``min_spanning_reads``, what the reference computes after ``new_block()``
    (``fell_back``: the caller starts its new block).  ``src``: anything with ``phase_relevant``."""
    return src.phase_relevant(index, cur_graph, prev_graph, prev_aligning, preds, 1 if start_of_block else 0, int(min_spanning_reads))


def bubble_from_relevant(rel: RelevantReads, ploidy: int, paths, read_sets) -> PackedBubble:
    """A ``PackedBubble`` from GLOBAL read ids: ``paths[p]`` the interior reads of path p (MergedReads expanded),
    ``read_sets[c][i]`` the reads of slot i of candidate c.  Ids go through ``rel.b_reads``; ids outside it can never match
    and are dropped, as ``pack_bubble`` drops the reads no alignment names."""
    b_reads = np.asarray(rel.b_reads, dtype=np.int64)

    def local(ids):
        ids = np.unique(np.asarray(list(ids), dtype=np.int64))
        at = np.searchsorted(b_reads, ids)
        ok = at < len(b_reads)
        ok[ok] = b_reads[at[ok]] == ids[ok]
        return at[ok].tolist()

    read_sets = [list(c) for c in read_sets]
    if not read_sets:
        raise ValueError("there must be at least one candidate set")
    if any(len(c) != ploidy for c in read_sets):
        raise ValueError("every candidate needs one read set per haplotype")
    path_off, path_ids = _csr([local(p) for p in paths])
    set_off, set_ids = _csr([local(s) for c in read_sets for s in c])
    out = PackedBubble(int(ploidy), len(paths), len(read_sets), len(rel.rel_reads), len(b_reads),
                       np.ascontiguousarray(rel.overlap_max, dtype=np.int32), np.ascontiguousarray(rel.aln_off, dtype=np.uint32),
                       np.ascontiguousarray(rel.aln_b, dtype=np.uint32), np.ascontiguousarray(rel.aln_a0, dtype=np.int32),
                       np.ascontiguousarray(rel.aln_a1, dtype=np.int32), path_off, path_ids, set_off, set_ids)
    out.b_reads = [int(x) for x in b_reads]
    return out


class HostIndex:
    """The contract of ``po_phase_index`` / ``po_phase_relevant`` in numpy, for machines without a GPU and for the tests; it is
    no fallback: nothing here picks it on its own.  ``lengths``: the length of every oriented read id."""

    def __init__(self, lengths):
        self.lengths = np.asarray(lengths, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.lengths)

    def phase_index(self, rows):
        """``rows``: structured (a_idx, b_idx, astart, aend, bstart, bend) or an int array [n, 6]."""
        rows = np.asarray(rows)
        if rows.dtype.names:
            rows = np.stack([rows[name].astype(np.int64) for name in rows.dtype.names], axis=1) if len(rows) else np.zeros((0, 6), np.int64)
        rows = rows.astype(np.int64).reshape(-1, 6)
        n, n_ids = len(rows), len(self)
        if 2 * n >= 2 ** 31:
            raise RuntimeError("po_phase_index: more than 2^30 - 1 rows in one call")
        if n and (rows[:, :2].min() < 0 or rows[:, :2].max() >= n_ids):
            raise ValueError("po_phase_index: a row names a read the handle does not hold")
        x, y, a0, a1 = (np.zeros(2 * n, dtype=np.int64) for _ in range(4))
        x[0::2], x[1::2], y[0::2], y[1::2] = rows[:, 0], rows[:, 1], rows[:, 1], rows[:, 0]
        a0[0::2], a1[0::2], a0[1::2], a1[1::2] = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
        key = (x << 32) | y
        order = np.lexsort((np.arange(2 * n), key))             # by key, then by sequence number
        last = np.ones(2 * n, dtype=bool)
        last[:-1] = key[order][1:] != key[order][:-1]           # the greatest sequence number of every key
        sel = order[last]
        entries = np.zeros(len(sel), dtype=ALIGNMENT_DTYPE)
        entries["b"], entries["a0"], entries["a1"], entries["seq"] = y[sel], a0[sel], a1[sel], sel
        off = np.searchsorted(x[sel], np.arange(n_ids + 1)).astype(np.uint64)
        return {"off": off, "entries": entries, "n_ids": n_ids}

    def phase_index_entries(self, index):
        return index["off"], index["entries"]

    def phase_relevant(self, index, cur_graph, prev_graph=(), prev_aligning=(), preds=(), mode: int = 0,
                       min_spanning_reads: int = 0) -> RelevantReads:
        off, entries, n_ids = index["off"], index["entries"], index["n_ids"]
        if mode not in (0, 1):
            raise ValueError("po_phase_relevant: the mode must be 0 (spanning) or 1 (all)")
        preds = [(int(p), int(e)) for p, e in preds]
        cur, prev_g, prev_a = (sorted({int(v) for v in l}) for l in (cur_graph, prev_graph, prev_aligning))
        if any(not 0 <= v < n_ids for l in (cur, prev_g, prev_a, [p for p, _ in preds]) for v in l) or n_ids != len(self):
            raise ValueError("po_phase_relevant: a list names a read the handle does not hold")
        u32, i32 = (lambda v: np.asarray(v, dtype=np.uint32)), (lambda v: np.asarray(v, dtype=np.int32))
        if not cur:
            return RelevantReads(u32([]), u32([]), i32([]), u32([0]), u32([]), i32([]), i32([]), u32([]), 0, False)
        seg = lambda v: entries[int(off[v]):int(off[v + 1])]   # noqa: E731
        ca = set(cur)
        for v in cur:
            ca.update(seg(v)["b"].tolist())
        spanning = ca & set(prev_a)
        fell_back = mode == 0 and len(spanning) < min_spanning_reads
        rel = sorted(spanning if mode == 0 and not fell_back else ca)
        G = np.asarray(sorted(set(cur) | (set() if fell_back else set(prev_g))), dtype=np.int64)
        om, aln_off, aln_b, a0, a1 = [], [0], [], [], []
        for r in rel:
            s = seg(r)
            at = np.searchsorted(G, s["b"])
            ok = at < len(G)
            ok[ok] = G[at[ok]] == s["b"][ok]
            aln_b += at[ok].tolist()
            a0 += s["a0"][ok].tolist()
            a1 += s["a1"][ok].tolist()
            aln_off.append(len(aln_b))
            m = int(self.lengths[r])
            for p, edge_len in preds:
                sp = seg(p)
                j = int(np.searchsorted(sp["b"], r))
                if j < len(sp) and int(sp["b"][j]) == r:
                    m = min(m, edge_len - int(sp["a0"][j]))
            om.append(m)
        return RelevantReads(u32(sorted(ca)), u32(rel), i32(om), u32(aln_off), u32(aln_b), i32(a0), i32(a1), u32(G), len(spanning), fell_back)


# ---- the walk along a bubble chain with resident candidates (po_walk_*) -----------------------------

Haploblock = namedtuple("Haploblock", "haplotypes read_sets include_last from_large_bubble log_rl tie")


def walk_paths(rel: RelevantReads, path_reads):
    """``(path_off, path_ids)`` of a step: the interior reads of every path as LOCAL ids of ``rel.b_reads`` (reads outside it
    can never match and are dropped, as in ``bubble_from_relevant``)."""
    b = bubble_from_relevant(rel, 1, path_reads, [[[]]])
    return b.path_off, b.path_ids


class HostWalk:
    """The contract of ``po_walk_*`` in numpy on a SCORER (a ``HostScorer``): the candidate sets of a walk as Python sets of
    global read ids, for machines without a GPU and for the tests.  Like ``HostScorer`` it is no fallback: nothing here picks
    it on its own."""

    def __init__(self, scorer, ploidy: int):
        if not 1 <= int(ploidy) <= 8:
            raise ValueError("po_walk_create: the ploidy must be 1 to 8")
        self.scorer, self.ploidy = scorer, int(ploidy)
        self._stats = {}
        self.reset()

    def reset(self) -> None:
        self._sets = [[set() for _ in range(self.ploidy)]]
        self._rl = [-math.inf]
        self._hist = [[]]
        self._block = set()
        # the resident route (po_walk_relevant, po_walk_step_resident): the two previous sets and the one live gather
        self._prev_graph, self._prev_aligning, self._route = set(), set(), 0
        live = getattr(self, "_live", None)
        if live is not None:
            if (live.fell_back or live.mode == 1) and live.resets == 0:   # (new_block(), then the step on the same relevant reads)
                live.resets, live.depth = 1, 0
            else:
                live.stale, self._live = True, None

    @property
    def start_of_block(self) -> bool:
        return not self._hist[0]

    def info(self) -> dict:
        depth = len(self._hist[0])
        return {"ploidy": self.ploidy, "n_cands": len(self._sets), "depth": depth, "start_of_block": int(depth == 0),
                "n_block_reads": len(self._block)}

    def phase_stats(self) -> dict:
        return self.scorer.phase_stats()

    def walk_stats(self) -> dict:
        return dict(self._stats)

    def step(self, rel: RelevantReads, path_reads, start_of_block, threshold: float = 0.0, min_spanning_reads: int = 0, levels=None,
             max_candidates: int = 0, advance: bool = True, cap: Optional[int] = None):
        if bool(start_of_block) != self.start_of_block:
            raise ValueError("po_walk_step: start_of_block is not the walk's")
        if self._route == 2:
            raise ValueError("po_walk_step: the block advanced by po_walk_step_resident: the two routes do not mix before po_walk_reset")
        cand, ext, rl = self._step(rel, path_reads, start_of_block, threshold, min_spanning_reads, levels, max_candidates, advance)
        if self._stats["advanced"]:
            self._route = 1
        n = len(rl) if cap is None else min(int(cap), len(rl))
        return cand[:n], ext[:n], rl[:n]

    def _step(self, rel: RelevantReads, path_reads, start_of_block, threshold, min_spanning_reads, levels, max_candidates, advance):
        b_reads = [int(x) for x in rel.b_reads]
        if any(y <= x for x, y in zip(b_reads, b_reads[1:])):
            raise ValueError("po_walk_step: b_reads is not strictly ascending")
        bubble = bubble_from_relevant(rel, self.ploidy, path_reads, self._sets)
        cand, ext, rl = self.scorer.phase_branch(bubble, start_of_block, min_spanning_reads, threshold, levels=levels,
                                                 max_candidates=max_candidates)
        n_in = len(self._sets)
        fresh = set(b_reads) - self._block
        advanced = bool(advance) and len(rl) > 0
        if advanced:
            inside = set(b_reads)
            interiors = [set(int(x) for x in p) & inside for p in path_reads]
            sets, hist = [], []
            for c, e in zip(cand.tolist(), ext.tolist()):
                digits = ext_digits(e, bubble.n_paths, self.ploidy)
                sets.append([self._sets[c][i] | interiors[d] for i, d in enumerate(digits)])
                hist.append(self._hist[c] + [int(e)])
            self._sets, self._hist, self._rl = sets, hist, [float(x) for x in rl]
            self._block |= fresh
        self._stats = {"n_cands_in": n_in, "n_cands_out": len(self._sets), "depth": len(self._hist[0]), "n_block_reads": len(self._block),
                       "n_new_reads": len(fresh), "words_per_slot": (len(self._block) + 31) // 32 if self._hist[0] else 0,
                       "advanced": int(advanced)}
        return cand, ext, rl

    def relevant(self, source, index, cur_graph, preds=(), start_of_block: bool = False, min_spanning_reads: int = 0,
                 without_prev_graph: bool = False) -> "HostGather":
        """``po_walk_relevant``: ``relevant_reads`` with ``prev_graph`` (empty with ``without_prev_graph``) and ``prev_aligning``
        taken from the walk.  The walk holds one live gather: this call makes the one before stale."""
        if self._route == 1:
            raise ValueError("po_walk_relevant: the block advanced by po_walk_step: the two routes do not mix before po_walk_reset")
        if getattr(self, "_live", None) is not None:
            self._live.stale = True
        cur_graph = [int(x) for x in cur_graph]
        rel = relevant_reads(source, index, cur_graph, [] if without_prev_graph else sorted(self._prev_graph), sorted(self._prev_aligning),
                             preds, start_of_block, min_spanning_reads)
        self._live = HostGather(rel, cur_graph, 1 if start_of_block else 0, len(self._hist[0]))
        return self._live

    def step_resident(self, rel: "HostGather", path_reads, start_of_block, threshold: float = 0.0, min_spanning_reads: int = 0, levels=None,
                      max_candidates: int = 0, advance: bool = True, cap: Optional[int] = None):
        """``po_walk_step_resident``: ``step`` on the live gather; a step that advances joins the gather's ``cur_graph`` to
        ``prev_graph`` and its ``cur_aligning`` to ``prev_aligning``."""
        if not isinstance(rel, HostGather):
            raise ValueError("po_walk_step_resident: needs the result of po_walk_relevant")
        if rel.stale or rel is not getattr(self, "_live", None):
            raise ValueError("po_walk_step_resident: the gather is stale: a later po_walk_relevant, a po_walk_reset or the freeing of "
                             "its walk has taken its arrays")
        if bool(start_of_block) != self.start_of_block:
            raise ValueError("po_walk_step_resident: start_of_block is not the walk's")
        if rel.depth != len(self._hist[0]):
            raise ValueError("po_walk_step_resident: the gather was made at another depth of the walk")
        if self._route == 1:
            raise ValueError("po_walk_step_resident: the block advanced by po_walk_step: the two routes do not mix before po_walk_reset")
        cand, ext, rl = self._step(rel.rel, path_reads, start_of_block, threshold, min_spanning_reads, levels, max_candidates, advance)
        if self._stats["advanced"]:
            self._route = 2
            self._prev_graph.update(rel.cur_graph)
            self._prev_aligning.update(int(x) for x in rel.rel.cur_aligning)
        n = len(rl) if cap is None else min(int(cap), len(rl))
        return cand[:n], ext[:n], rl[:n]

    def prev_sets(self):
        """``po_walk_prev_copy``: ``(prev_graph, prev_aligning)`` as ascending lists."""
        return sorted(self._prev_graph), sorted(self._prev_aligning)

    def best(self):
        """``prune(candidate_sets, 1.0)``: ``(candidates, greatest log_rl)``."""
        top = max(self._rl)
        if len(self._rl) < 2 or top == -math.inf:
            return list(range(len(self._rl))), top
        return [j for j, x in enumerate(self._rl) if x - top >= 0.0], top

    def _named(self, cands):
        cands = [int(c) for c in cands]
        if any(not 0 <= c < len(self._sets) for c in cands):
            raise ValueError("a candidate is not below the number the walk holds")
        return cands

    def history(self, cands) -> np.ndarray:
        cands = self._named(cands)
        return np.asarray([self._hist[c] for c in cands], dtype=np.uint32).reshape(len(cands), len(self._hist[0]))

    def read_sets(self, cands) -> list:
        return [[sorted(s) for s in self._sets[c]] for c in self._named(cands)]

    def close(self) -> None:
        pass


class HostGather:
    """What ``HostWalk.relevant`` returns: the sizes of the gather as attributes, ``fetch()`` for the arrays, ``close()``."""

    def __init__(self, rel: RelevantReads, cur_graph, mode: int, depth: int):
        self.rel, self.cur_graph, self.mode, self.depth = rel, list(cur_graph), int(mode), int(depth)
        self.stale, self.resets = False, 0
        self.n_cur_aligning, self.n_spanning, self.n_relevant = len(rel.cur_aligning), int(rel.n_spanning), len(rel.rel_reads)
        self.n_alignments, self.n_b, self.fell_back = len(rel.aln_b), len(rel.b_reads), bool(rel.fell_back)

    def fetch(self) -> RelevantReads:
        if self.stale:
            raise ValueError("po_relevant_copy: the gather is stale: a later po_walk_relevant, a po_walk_reset or the freeing of its "
                             "walk has taken its arrays")
        return self.rel

    def close(self) -> None:
        pass


def chain_bubbles_input(bubble_paths: "BubblePaths", chain: int, reads_of_node: Callable, is_merged: Optional[Callable] = None,
                        resident_above: Optional[int] = None) -> List[dict]:
    """The bubbles of one chain in the order of the walk, as ``phase_chain`` takes them: ``entrance``, ``exit``, ``paths``
    (node tuples, both ends included), ``interior_nodes``, ``interior_reads`` (MergedReads expanded through
    ``reads_of_node(node) -> read ids``, every read once) and ``preds`` (the predecessors of the exit that are plain reads, as
    read ids, with their edge lengths: a merged predecessor is no key of the alignments and is left out).  ``is_merged(node)``:
    default, a node is merged unless ``reads_of_node`` gives the node itself (node ids that are read ids).
    ``resident_above`` (with a ``DevicePaths`` or a ``HostResidentPaths``): the paths of a bubble with more paths than this
    stay where they are -- its ``paths`` is None, ``n_paths`` the count and ``scorer`` a ``ResidentBubble`` that
    ``phase_chain`` asks at its large arm."""
    if is_merged is None:
        is_merged = lambda x: [int(r) for r in reads_of_node(x)] != [int(x)]   # noqa: E731
    out = []
    for b in bubble_paths.chain_bubbles(chain):
        inside = bubble_paths.interior_of(b)
        preds = [(int(list(reads_of_node(p))[0]), int(weight)) for p, weight in bubble_paths.preds_of(b) if not is_merged(p)]
        if resident_above is not None and bubble_paths.is_listed(b) and bubble_paths.is_large(b, resident_above):
            out.append({"entrance": int(bubble_paths.bubbles["entrance"][b]), "exit": int(bubble_paths.bubbles["exit"][b]), "paths": None,
                        "n_paths": int(bubble_paths.bubbles["n_paths"][b]), "scorer": ResidentBubble(bubble_paths, b),
                        "interior_nodes": [int(x) for x in inside],
                        "interior_reads": list(dict.fromkeys(int(r) for x in inside for r in reads_of_node(x))), "preds": preds})
            continue
        out.append({"entrance": int(bubble_paths.bubbles["entrance"][b]), "exit": int(bubble_paths.bubbles["exit"][b]),
                    "paths": [tuple(int(x) for x in p) for p in bubble_paths.paths_of(b)], "interior_nodes": [int(x) for x in inside],
                    "interior_reads": list(dict.fromkeys(int(r) for x in inside for r in reads_of_node(x))), "preds": preds})
    return out


def phase_chain(scorer, source, index, bubbles, reads_of_node: Callable, ploidy: int, min_spanning_reads: int = 3, max_bubble_size: int = 10,
                threshold=1e-3, prune_factor=0.1, max_candidates: int = 500, max_prune_rounds: int = 9, prune_step_size: float = 0.1,
                walk=None, choose: Callable = random.choice, on_step: Optional[Callable] = None, large_scores: bool = False,
                resident: bool = False):
    """``BubbleChainPhaser.phase()`` (phasm/phasing.py:182-364) over ``bubbles`` (``chain_bubbles_input``), arm by arm, as a
    generator of ``Haploblock``.  ``scorer``: what ``score_paths`` needs at a large bubble; ``source`` / ``index``: what
    ``relevant_reads`` needs; ``walk``: a ``DeviceWalk`` (``ExactOverlapper.phase_walk``) or a ``HostWalk`` -- None: the
    scorer's own ``phase_walk(ploidy)``, closed at the end.  ``threshold`` (of the number of relevant reads) and
    ``prune_factor`` (of the length of the kept list) may be callables.  ``choose`` picks one candidate of a tie set (a list of
    candidate numbers).  ``on_step`` receives one dict per turn of the loop (the keys of a trace step of tests/walk_utils.py that the walk knows
    without extra device work, and under ``steps`` the raw ``(cand, ext, rl)`` of every step call) and one with ``final`` at the
    end (``prune_in``, the advanced bubbles of the last block, the two host sets).
    A bubble whose ``paths`` is absent or None keeps them elsewhere (``chain_bubbles_input`` with ``resident_above``): it
    gives ``n_paths`` and a ``scorer`` with ``score_large(rel, reads_of_node, n_best, want_scores)`` and ``path_of(p)``.  At
    the large arm that scorer is asked with the relevant reads and only the winner's node tuple is fetched; ``on_step`` gets
    ``best``, ``winner`` and ``arm``, and ``scores`` only with ``large_scores``.  Such a bubble that is NOT large cannot be
    walked (the branch arm needs its paths on the host, at most 64 of them): ``ValueError`` naming the bubble.
    ``prev_graph_reads`` and ``prev_aligning_reads`` are host sets -- unless ``resident``: then they are the walk's
    (``walk.relevant`` / ``walk.step_resident`` / ``walk.prev_sets``), the loop keeps none of its own and
    the arrays of the relevant reads come to the host only where they are needed there: at the large arm and, for the keys of
    the trace, when ``on_step`` is given.  Arms, yields and error sentences are the same.  One difference from the reference: a bubble that keeps no
    candidate even as the start of a block makes the reference loop for ever; here it raises ``ValueError``."""
    k = int(ploidy)
    own = walk is None
    if own:
        walk = scorer.phase_walk(k)
    if walk.info()["ploidy"] != k:
        raise ValueError("the walk's ploidy is not %d" % k)
    prev_graph, prev_aligning, block_paths, block_bubbles = set(), set(), [], []
    expand = lambda nodes: [int(r) for x in nodes for r in reads_of_node(x)]   # noqa: E731

    def as_yield(block, kind):
        return {"kind": kind, "include_last": int(block.include_last), "tie": block.tie, "haplotypes": block.haplotypes,
                "read_sets": block.read_sets}

    def best_block(include_last):
        tie, top = walk.best()
        pick = int(choose(list(tie)))
        haplotypes = [[] for _ in range(k)]
        for paths, e in zip(block_paths, walk.history([pick]).reshape(-1).tolist()):
            for h, d in zip(haplotypes, ext_digits(e, len(paths), k)):
                path = list(paths[d])
                h.extend(path[1:] if h and h[-1] == path[0] else path)
        return Haploblock(haplotypes, walk.read_sets([pick])[0], include_last, False, float(top), [int(c) for c in tie])

    def new_block():
        block = best_block(False)
        walk.reset()
        prev_graph.clear()        # (with `resident` the two stay empty: the sets are the walk's)
        prev_aligning.clear()
        del block_paths[:], block_bubbles[:]
        return block

    gather = None
    try:
        i = 0
        while i < len(bubbles):
            if gather is not None:
                gather.close()
                gather = None
            b = bubbles[i]
            on_device = b.get("paths") is None
            if on_device:
                n_here = int(b["n_paths"])
                if n_here <= max_bubble_size:
                    raise ValueError("bubble %d (%s .. %s) has %d paths that are not on the host: only a large bubble (more than "
                                     "max_bubble_size = %d paths) is scored where its paths are" %
                                     (i, b.get("entrance"), b.get("exit"), n_here, max_bubble_size))
                paths, path_reads = None, None
            else:
                paths = [tuple(p) for p in b["paths"]]
                path_reads = [expand(path[1:-1]) for path in paths]
                n_here = len(paths)
            start = walk.start_of_block
            s = {"bubble": i, "start": int(start), "arm": "skipped", "broke": 0, "fell_back": 0, "yields": [], "steps": []}
            large = n_here > max_bubble_size
            if resident:
                gather = walk.relevant(source, index, b["interior_reads"], b["preds"], start or large, 0 if large else min_spanning_reads,
                                       without_prev_graph=large)
                rel = gather.fetch() if large or on_step else None   # (before new_block() below: a reset may make the gather stale)
                n_rel, n_aln, fell_back = gather.n_relevant, gather.n_alignments, gather.fell_back
            else:
                rel = relevant_reads(source, index, b["interior_reads"], [] if large else sorted(prev_graph), sorted(prev_aligning), b["preds"],
                                     start or large, 0 if large else min_spanning_reads)
                n_rel, n_aln, fell_back = len(rel.rel_reads), len(rel.aln_b), rel.fell_back
            if rel is not None:
                s.update({"cur_aligning": rel.cur_aligning.tolist(), "n_spanning": int(rel.n_spanning), "rel_reads": rel.rel_reads.tolist(),
                          "overlap_max": rel.overlap_max.tolist(), "aln_off": rel.aln_off.tolist(),
                          "aln_y": [int(rel.b_reads[x]) for x in rel.aln_b.tolist()], "aln_a0": rel.aln_a0.tolist(),
                          "aln_a1": rel.aln_a1.tolist(), "n_b": len(rel.b_reads)})
            if (large and not start) or fell_back:
                block = new_block()
                s["yields"].append(as_yield(block, "new_block"))
                s["broke"], s["fell_back"] = 1, int(fell_back)
                yield block
                start = True
            if large and on_device:
                best, _, scores = b["scorer"].score_large(rel, reads_of_node, k, want_scores=large_scores)
                if scores is not None:
                    s["scores"] = np.asarray(scores).tolist()
                s["best"], s["winner"], s["arm"] = [int(p) for p in best], int(best[0]), "large"
                winner = tuple(int(x) for x in b["scorer"].path_of(s["winner"]))
                block = Haploblock([list(winner)] + [[] for _ in range(k - 1)],
                                   [sorted(set(expand(winner[1:-1])))] + [[] for _ in range(k - 1)], False, True, -math.inf, None)
                s["yields"].append(as_yield(block, "large"))
                if on_step:
                    on_step(s)
                yield block
                i += 1
                continue
            if large:
                scores = score_paths(scorer, bubble_from_relevant(rel, k, path_reads, [[[] for _ in range(k)]]))
                s["scores"], s["best"] = scores.tolist(), best_paths(scores, k)
                s["winner"], s["arm"] = s["best"][0], "large"
                block = Haploblock([list(paths[s["winner"]])] + [[] for _ in range(k - 1)],
                                   [sorted(set(path_reads[s["winner"]]))] + [[] for _ in range(k - 1)], False, True, -math.inf, None)
                s["yields"].append(as_yield(block, "large"))
                if on_step:
                    on_step(s)
                yield block
                i += 1
                continue
            if n_aln == 0:
                if on_step:
                    on_step(s)
                i += 1
                continue
            R = n_rel
            level = threshold(R) if callable(threshold) else threshold
            step = (lambda *a, **kw: walk.step_resident(gather, *a, **kw)) if resident else (lambda *a, **kw: walk.step(rel, *a, **kw))
            factor = prune_factor
            s["n_cands_in"] = walk.info()["n_cands"]
            if callable(factor):
                cand, ext, rl = step(path_reads, start, level, min_spanning_reads, levels=None, advance=False)
                s["kept_cand"], s["kept_ext"], s["kept_rl"] = cand.tolist(), ext.tolist(), rl.tolist()
                s["steps"].append((cand, ext, rl))
                factor = factor(len(rl)) if len(rl) >= 2 else 0.0
            cand, ext, rl = step(path_reads, start, level, min_spanning_reads,
                                 levels=prune_levels(float(factor), float(prune_step_size), int(max_prune_rounds)),
                                 max_candidates=int(max_candidates), advance=True)
            s["steps"].append((cand, ext, rl))
            s["phase_stats"] = walk.phase_stats()
            s["n_kept"] = int(s["phase_stats"]["n_kept"])
            s["prune_factor"] = None if s["n_kept"] < 2 else float(factor)
            s["surv_cand"], s["surv_ext"], s["surv_rl"] = cand.tolist(), ext.tolist(), rl.tolist()
            s["arm"] = "advanced"
            if len(rl):
                block_paths.append(paths)
                block_bubbles.append(i)
                if not resident:
                    prev_graph.update(int(r) for r in b["interior_reads"])
                    prev_aligning.update(s["cur_aligning"])
                if on_step:
                    on_step(s)
                i += 1
                continue
            if start:
                raise ValueError("bubble %d (%s .. %s) keeps no candidate even as the start of a block" % (i, b.get("entrance"), b.get("exit")))
            block = new_block()
            s["yields"].append(as_yield(block, "new_block"))
            s["arm"] = "retry"
            if on_step:
                on_step(s)
            yield block
        if gather is not None:
            gather.close()
            gather = None
        held = walk.prev_sets() if resident else (sorted(prev_graph), sorted(prev_aligning))
        final = {"final": True, "yields": [], "block_bubbles": list(block_bubbles), "prev_graph": list(held[0]),
                 "prev_aligning": list(held[1])}
        if not walk.start_of_block:
            final["prune_in"] = walk.info()["n_cands"]
            block = best_block(True)
            final["yields"].append(as_yield(block, "final"))
            if on_step:
                on_step(final)
            yield block
        elif on_step:
            on_step(final)
    finally:
        if gather is not None:
            gather.close()
        if own:
            walk.close()


# ---- every listed path of a large bubble scored where it is (po_phase_large) -------------------------

def large_node_lists(rel: RelevantReads, interior_nodes, reads_of_node: Callable):
    """``(node_off, node_ids)`` of ``po_phase_large``: per interior node, in the order given, the LOCAL ids (places in
    ``rel.b_reads``) of its reads, ascending, every read once; reads outside ``rel.b_reads`` can never match and are dropped."""
    b_reads = np.asarray(rel.b_reads, dtype=np.int64)
    lists = []
    for node in interior_nodes:
        ids = np.unique(np.asarray([int(r) for r in reads_of_node(node)], dtype=np.int64))
        at = np.searchsorted(b_reads, ids)
        ok = at < len(b_reads)
        ok[ok] = b_reads[at[ok]] == ids[ok]
        lists.append(at[ok].tolist())
    return _csr(lists)


def best_of_scores(scores: np.ndarray, n_best: int) -> List[int]:
    """``best_paths`` without a Python sort over every path: descending by score, among equal scores the lower index first."""
    scores = np.asarray(scores, dtype=np.float64)
    order = np.lexsort((np.arange(len(scores)), -scores))
    return [int(p) for p in order[:int(n_best)]]


def host_score_large(rel: RelevantReads, node_off, node_ids, interior_nodes, paths) -> np.ndarray:
    """The scores of ``po_phase_large`` in numpy: the interval of every (interior node, read), joined along every path with min
    and max, ``f`` summed over the reads and divided by their number.  ``paths``: node tuples with both ends."""
    R = len(rel.rel_reads)
    if R == 0:
        raise ZeroDivisionError("no relevant reads")
    n_inside = len(interior_nodes)
    as_sets = PackedBubble(1, n_inside, 1, R, len(rel.b_reads), np.asarray(rel.overlap_max, dtype=np.int32), np.asarray(rel.aln_off, dtype=np.uint32),
                           np.asarray(rel.aln_b, dtype=np.uint32), np.asarray(rel.aln_a0, dtype=np.int32), np.asarray(rel.aln_a1, dtype=np.int32),
                           np.asarray(node_off, dtype=np.uint32), np.asarray(node_ids, dtype=np.uint32), np.zeros(2, np.uint32), np.zeros(0, np.uint32))
    s0, e = HostScorer._intervals(as_sets, as_sets.path_off, as_sets.path_ids, n_inside)
    s0 = np.vstack([s0, np.full((1, R), NO_START, dtype=np.int64)])      # (slot n_inside: no node)
    e = np.vstack([e, np.zeros((1, R), dtype=np.int64)])
    slot = {int(x): j for j, x in enumerate(interior_nodes)}
    om = np.asarray(rel.overlap_max, dtype=np.float64)
    out = np.zeros(len(paths), dtype=np.float64)
    step = max(1, (1 << 22) // max(1, R))                                  # (paths per block: about 32 MB of joins at a time)
    for lo in range(0, len(paths), step):
        block = paths[lo:lo + step]
        longest = max([len(p) - 2 for p in block] + [1])
        idx = np.full((len(block), longest), n_inside, dtype=np.int64)
        for j, p in enumerate(block):
            inner = [slot[int(x)] for x in tuple(p)[1:-1] if int(x) in slot]
            idx[j, :len(inner)] = inner
        ps0, pe = np.full((len(block), R), NO_START, dtype=np.int64), np.zeros((len(block), R), dtype=np.int64)
        for c in range(longest):
            ps0 = np.minimum(ps0, s0[idx[:, c]])
            pe = np.maximum(pe, e[idx[:, c]])
        with np.errstate(divide="ignore", invalid="ignore"):
            out[lo:lo + len(block)] = np.where(ps0 < pe, (pe - ps0) / om[None, :], 0.0).sum(axis=1) / R
    return out


class ResidentBubble:
    """One bubble of a ``DevicePaths`` or ``HostResidentPaths``: what ``phase_chain`` asks at the large arm of a bubble whose
    paths are not on the host."""

    def __init__(self, src, b: int):
        self.src, self.b = src, int(b)

    def score_large(self, rel: RelevantReads, reads_of_node: Callable, n_best: int, want_scores: bool = False):
        return self.src.score_large(self.b, rel, reads_of_node, n_best, want_scores=want_scores)

    def path_of(self, p: int) -> tuple:
        return self.src.path_of(self.b, p)


# ---- paths, interior and exit predecessors of every top-level bubble (po_phase_paths) ---------------

@dataclass
class BubblePaths:
    """What ``po_phase_paths`` gives: one table entry per top-level bubble, ordered by (chain, position), and CSR arrays.
    ``bubbles``: BUBBLE_PATHS_DTYPE (entrance, exit, chain, position, n_inside, flags, n_paths, n_path_nodes)."""
    bubbles: np.ndarray            # BUBBLE_PATHS_DTYPE [B]
    inside_off: np.ndarray         # uint64 [B + 1] into inside_nodes
    inside_nodes: np.ndarray       # uint32: interior nodes, ascending in rank of the node order
    pred_off: np.ndarray           # uint64 [B + 1] into pred_node / pred_weight
    pred_node: np.ndarray          # uint32: the predecessors of the exit, in the graph's edge order
    pred_weight: np.ndarray        # int32: g[pred][exit]['weight']
    bubble_path_off: np.ndarray    # uint64 [B + 1]: the number of the bubble's first listed path
    path_off: np.ndarray           # uint64 [P + 1] into path_nodes
    path_nodes: np.ndarray         # uint32: the listed paths, both ends included

    def __len__(self) -> int:
        return len(self.bubbles)

    def is_listed(self, b: int) -> bool:
        return not int(self.bubbles["flags"][b]) & PATHS_UNLISTED

    def is_bare(self, b: int) -> bool:
        return bool(int(self.bubbles["flags"][b]) & PATHS_BARE)

    def paths_of(self, b: int) -> List[tuple]:
        """``[tuple(p) for p in networkx.all_simple_paths(g, entrance, exit)]`` of bubble b, in that order."""
        if not self.is_listed(b):
            raise ValueError("bubble %d has %s paths: more than max_paths, they were not listed" % (b, paths_text(self.bubbles["n_paths"][b])))
        off, nodes = self.path_off, self.path_nodes
        return [tuple(nodes[int(off[p]):int(off[p + 1])].tolist())
                for p in range(int(self.bubble_path_off[b]), int(self.bubble_path_off[b + 1]))]

    def interior_of(self, b: int) -> List[int]:
        """``superbubble_nodes(g, entrance, exit) - {entrance, exit}`` of bubble b, in node order."""
        return self.inside_nodes[int(self.inside_off[b]):int(self.inside_off[b + 1])].tolist()

    def preds_of(self, b: int) -> List[tuple]:
        """``[(p, g[p][exit]['weight']) for p in g.predecessors_iter(exit)]`` of bubble b, in the graph's edge order."""
        lo, hi = int(self.pred_off[b]), int(self.pred_off[b + 1])
        return list(zip(self.pred_node[lo:hi].tolist(), self.pred_weight[lo:hi].tolist()))

    def chain_bubbles(self, chain: int) -> List[int]:
        """The bubbles ``phase()`` visits on chain ``chain``, in its order: those of the chain by position, up to the first
        bare one (``non_branching_bubble`` drops it, and ``while entrance in self.bubble_entrances`` ends there)."""
        out = []
        for b in np.flatnonzero(self.bubbles["chain"] == chain).tolist():   # (the table is ordered by (chain, position))
            if self.is_bare(b):
                break
            out.append(b)
        return out

    def is_large(self, b: int, max_bubble_size: int) -> bool:
        """``len(possible_paths) > max_bubble_size``, from the count alone."""
        return int(self.bubbles["n_paths"][b]) > int(max_bubble_size)


def paths_text(n_paths) -> str:
    """A path count as the tools print it: a saturated one as a lower bound."""
    return ">=2^64-1" if int(n_paths) == PATHS_MANY else str(int(n_paths))


class HostResidentPaths(BubblePaths):
    """The interface of ``ExactOverlapper.phase_paths_resident`` (a ``DevicePaths``) in numpy over a ``BubblePaths`` whose
    paths are all on the host: for machines without a GPU and for the tests.  It is no fallback: nothing here picks it on its
    own.  The same decomposition over the interior nodes and the same tie rule; the order of its float64 sums may differ."""

    def __init__(self, listed: BubblePaths):
        super().__init__(listed.bubbles, listed.inside_off, listed.inside_nodes, listed.pred_off, listed.pred_node, listed.pred_weight,
                         listed.bubble_path_off, listed.path_off, listed.path_nodes)
        self._stats = {}

    def path_of(self, b: int, p: int) -> tuple:
        first, n = int(self.bubble_path_off[b]), int(self.bubble_path_off[b + 1]) - int(self.bubble_path_off[b])
        if not self.is_listed(b) or not 0 <= int(p) < n:
            raise ValueError("bubble %d has no listed path %d" % (b, p))
        g = first + int(p)
        return tuple(self.path_nodes[int(self.path_off[g]):int(self.path_off[g + 1])].tolist())

    def score_large(self, b: int, rel: RelevantReads, reads_of_node: Callable, n_best: int, want_scores: bool = False):
        """``(best, best_scores, scores or None)``: what ``po_phase_large`` gives for bubble b."""
        if not 1 <= int(n_best) <= 8:
            raise ValueError("po_phase_large: n_best must be 1 to 8")
        paths = self.paths_of(b)
        inside = self.interior_of(b)
        node_off, node_ids = large_node_lists(rel, inside, reads_of_node)
        scores = host_score_large(rel, node_off, node_ids, inside, paths)
        best = best_of_scores(scores, n_best)
        self._stats = {"n_paths": len(paths), "n_inside": len(inside), "n_reads": len(rel.rel_reads),
                       "max_path_nodes": max([len(p) for p in paths] + [0])}
        return best, scores[best].copy(), (scores if want_scores else None)

    def large_stats(self) -> dict:
        return dict(self._stats)

    def close(self) -> None:
        pass


def bubble_paths(src, graph, max_paths: int = 0) -> BubblePaths:
    """``src.phase_paths(graph, max_paths)``: ``src`` is an ``ExactOverlapper`` with one of its graph results, or a ``HostPaths``
    (then ``graph`` is ignored: it holds its own)."""
    return src.phase_paths(graph, max_paths)


class HostPaths:
    """``po_phase_paths`` in plain Python / numpy, on ``edges`` (rows that start with u, v, weight) and the graph's node
    order: for machines without a GPU and for the tests.  It is no fallback: nothing here picks it on its own.  The bubbles
    are found the way the device finds them (DESIGN.md sections 3.9j, 3.9k): the singleton SCCs, immediate dominators and
    post-dominators of their DAG under one virtual root and one virtual sink, the pairs (s, t) with t = ipdom[s] and
    s = idom[t], the discards for self-loops, the top-level ones, their chains."""

    def __init__(self, edges, node_order):
        e = np.asarray(edges, dtype=np.int64).reshape(len(edges), -1) if len(edges) else np.zeros((0, 3), np.int64)
        self.order = [int(x) for x in node_order]
        rank = {x: r for r, x in enumerate(self.order)}
        if len(rank) != len(self.order):
            raise ValueError("po_phase_paths: the node order repeats a node")
        try:
            self.eu = [rank[int(u)] for u in e[:, 0]]
            self.ev = [rank[int(v)] for v in e[:, 1]]
        except KeyError:
            raise ValueError("po_phase_paths: an edge has an end that is not in the node order")
        self.weight = e[:, 2].tolist() if e.shape[1] > 2 else [0] * len(e)
        n = len(self.order)
        self.succ = [[] for _ in range(n)]       # (head rank, edge index), in edge order
        self.pred = [[] for _ in range(n)]
        for k, (a, b) in enumerate(zip(self.eu, self.ev)):
            self.succ[a].append((b, k))
            self.pred[b].append((a, k))
        self._bubbles()
        self.stats = {}

    def _sccs(self):
        """Tarjan, iterative: the SCC number of every rank."""
        n = len(self.order)
        index, low, comp, on = [-1] * n, [0] * n, [-1] * n, [False] * n
        stack, count, n_comp = [], 0, 0
        for root in range(n):
            if index[root] != -1:
                continue
            work = [(root, 0)]
            while work:
                v, i = work.pop()
                if i == 0:
                    index[v] = low[v] = count
                    count += 1
                    stack.append(v)
                    on[v] = True
                if i < len(self.succ[v]):
                    w = self.succ[v][i][0]
                    work.append((v, i + 1))
                    if index[w] == -1:
                        work.append((w, 0))
                    elif on[w]:
                        low[v] = min(low[v], index[w])
                    continue
                if low[v] == index[v]:
                    while True:
                        w = stack.pop()
                        on[w] = False
                        comp[w] = n_comp
                        if w == v:
                            break
                    n_comp += 1
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
        return comp, n_comp

    @staticmethod
    def _idoms(n, parents, topo):
        """Immediate dominators on a DAG with root n (``parents[v]`` empty: v hangs on the root), in topological order."""
        idom, depth = [n] * (n + 1), [0] * (n + 1)
        for v in topo:
            ps = parents[v]
            a = ps[0] if ps else n
            for b in ps[1:]:
                while a != b:
                    if depth[a] >= depth[b]:
                        a = idom[a]
                    else:
                        b = idom[b]
            idom[v], depth[v] = a, depth[a] + 1
        return idom

    def _bubbles(self):
        n = len(self.order)
        comp, n_comp = self._sccs()
        size = [0] * n_comp
        for c in comp:
            size[c] += 1
        real = [size[comp[r]] == 1 for r in range(n)]
        loop = [False] * n
        parents, children = [[] for _ in range(n)], [[] for _ in range(n)]
        from_root, to_sink = [False] * n, [False] * n
        for a, b in zip(self.eu, self.ev):
            if a == b:
                loop[a] = True
            elif real[a] and real[b]:
                parents[b].append(a)
                children[a].append(b)
            else:
                from_root[b] = from_root[b] or not real[a]
                to_sink[a] = to_sink[a] or not real[b]
        reals = [r for r in range(n) if real[r]]
        indeg = {r: len(parents[r]) for r in reals}
        topo = [r for r in reals if indeg[r] == 0]
        for v in topo:
            for c in children[v]:
                indeg[c] -= 1
                if indeg[c] == 0:
                    topo.append(c)
        idom = self._idoms(n, [[] if from_root[r] else parents[r] for r in range(n)], topo)
        ipdom = self._idoms(n, [[] if to_sink[r] else children[r] for r in range(n)], topo[::-1])
        cand = {s: ipdom[s] for s in reals if ipdom[s] < n and idom[ipdom[s]] == s}
        interior = {}
        for s, t in cand.items():                # the nodes reached from s without passing t
            seen, todo = {s, t}, [s]
            while todo:
                for w, _ in self.succ[todo.pop()]:
                    if w not in seen:
                        seen.add(w)
                        todo.append(w)
            interior[s] = seen - {s, t}
        alive = {s: t for s, t in cand.items() if not (loop[s] or loop[t] or any(loop[x] for x in interior[s]))}
        held = set().union(*[interior[s] for s in alive]) if alive else set()
        self.top = {s: t for s, t in alive.items() if s not in held}
        self.interior = {s: sorted(interior[s]) for s in self.top}
        exits = set(self.top.values())
        self.table = []                          # (entrance rank, chain, position), by (chain, position)
        for chain, head in enumerate(s for s in sorted(self.top) if s not in exits):
            s, position = head, 0
            while s in self.top:
                self.table.append((s, chain, position))
                s, position = self.top[s], position + 1

    def _counts(self, s):
        """cnt of every member of the bubble that s enters, saturating."""
        t, members = self.top[s], [s] + self.interior[s]
        inside = set(self.interior[s])
        cnt, stray = {}, 0
        todo = [(s, 0)]
        while todo:                              # post-order over the members
            v, i = todo.pop()
            if i < len(self.succ[v]):
                todo.append((v, i + 1))
                w = self.succ[v][i][0]
                if w != t and w in inside and w not in cnt:
                    todo.append((w, 0))
                continue
            total = 0
            for w, _ in self.succ[v]:
                if w == t:
                    total += 1
                elif w in inside:
                    total += cnt[w]
                else:
                    stray += 1
            cnt[v] = min(total, PATHS_MANY)
        for v in members:                        # (a member that no path from s reaches: cannot happen in a superbubble)
            cnt.setdefault(v, 0)
        return cnt, stray

    def _unrank(self, s, cnt, j):
        t, inside, path, v = self.top[s], set(self.interior[s]), [s], s
        while v != t:
            for w, _ in self.succ[v]:
                c = 1 if w == t else (cnt[w] if w in inside else 0)
                if j < c:
                    break
                j -= c
            else:
                raise RuntimeError("the counts of bubble %d do not add up" % self.order[s])
            path.append(w)
            v = w
        return path

    def phase_paths(self, graph=None, max_paths: int = 0) -> BubblePaths:
        if not 0 <= int(max_paths) < 2**64:
            raise ValueError("max_paths does not fit 64 bits")
        order = self.order
        table = np.zeros(len(self.table), dtype=BUBBLE_PATHS_DTYPE)
        inside_off, pred_off, bpo, path_off = [0], [0], [0], [0]
        inside_nodes, pred_node, pred_weight, path_nodes = [], [], [], []
        n_stray, n_listed = 0, 0
        for b, (s, chain, position) in enumerate(self.table):
            t = self.top[s]
            cnt, stray = self._counts(s)
            n_stray += stray
            n_paths = cnt[s]
            saturated = n_paths == PATHS_MANY
            unlisted = saturated or n_paths > max_paths
            n_listed += 0 if unlisted else n_paths
            if n_listed >= 2**30:
                raise OverflowError("po_phase_paths: at least %d paths to list in one call, at most 2^30 - 1" % n_listed)
            first = len(path_nodes)
            if not unlisted:
                for j in range(n_paths):
                    path_nodes += [order[v] for v in self._unrank(s, cnt, j)]
                    path_off.append(len(path_nodes))
                if len(path_nodes) >= 2**31:
                    raise OverflowError("po_phase_paths: the listed paths hold %d nodes together, at most 2^31 - 1" % len(path_nodes))
            flags = (PATHS_BARE if not self.interior[s] else 0) | (PATHS_UNLISTED if unlisted else 0) | (PATHS_SATURATED if saturated else 0)
            table[b] = (order[s], order[t], chain, position, len(self.interior[s]), flags, n_paths, len(path_nodes) - first)
            inside_nodes += [order[v] for v in self.interior[s]]
            inside_off.append(len(inside_nodes))
            for p, k in self.pred[t]:
                pred_node.append(order[p])
                pred_weight.append(self.weight[k])
            pred_off.append(len(pred_node))
            bpo.append(len(path_off) - 1)
        u64, u32 = (lambda v: np.asarray(v, dtype=np.uint64)), (lambda v: np.asarray(v, dtype=np.uint32))
        flags = table["flags"]
        self.stats = {"n_nodes": len(order), "n_edges": len(self.eu), "n_invalid": 0, "n_bubbles": len(table),
                      "n_bare": int((flags & PATHS_BARE != 0).sum()), "n_unlisted": int((flags & PATHS_UNLISTED != 0).sum()),
                      "n_saturated": int((flags & PATHS_SATURATED != 0).sum()), "n_listed_paths": len(path_off) - 1,
                      "n_path_nodes": len(path_nodes), "max_paths_seen": int(table["n_paths"].max()) if len(table) else 0,
                      "max_path_nodes": int(np.diff(path_off).max()) if len(path_off) > 1 else 0, "n_stray_edges": n_stray}
        return BubblePaths(table, u64(inside_off), u32(inside_nodes), u64(pred_off), u32(pred_node), np.asarray(pred_weight, dtype=np.int32),
                           u64(bpo), u64(path_off), u32(path_nodes))

    def paths_stats(self) -> dict:
        return dict(self.stats)
