"""Drop-in for the reference's ``phasm.overlapper`` extension module.

The reference exposes, through pybind11 (/root/reference/src/phasm.cpp:8-18)::

    class ExactOverlapper:
        def __init__(self)                       # src/overlapper.cpp:19
        def add_sequence(self, id: str, seq: str) -> None      # src/overlapper.cpp:22-26
        def overlaps(self, min_length: int) -> List[Tuple[str, str, int, int, int, int]]
                                                                # src/overlapper.cpp:28-150

and ``phasm overlap`` is its only caller (phasm/cli/assembler.py:31,39-42).  This class has
the same three methods with the same argument meaning, return type and error behaviour
(negative ``min_length`` -> ``TypeError`` like pybind11's unsigned conversion; ``bytes`` ids
and sequences accepted like pybind11's ``std::string`` caster), and calls the HIP library
through the C ABI of include/phasm_overlap.h.  Extra, non-reference methods
(``overlaps_array``, ``overlaps_shard_array``, ``stats``) expose the bulk 24-byte row array
so callers that want throughput do not have to build millions of Python tuples.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import CAND_DTYPE, CONTIG_DTYPE, EDGE_DTYPE, PoContigParams, PoContigStats, ROW_DTYPE, PoLayoutParams, PoLayoutStats, PoNodeOrderStats, PoReduceParams, PoReduceStats, PoStats, PoTipsParams, PoTipsStats, PoDiamondParams, PoDiamondStats, PoMergeParams, PoMergeStats, PoCoverageParams, PoCoverageStats, COVERAGE_DTYPE, PoComponentsParams, PoComponentsStats, COMPONENT_DTYPE, PoPartitionParams, PoPartitionStats, SCC_DTYPE, PoSuperbubbleParams, PoSuperbubbleStats, PoSuperbubbleAllParams, PoSuperbubbleAllStats, SUPERBUBBLE_DTYPE, PoBubblechainParams, PoBubblechainStats, PoBubblechainAllStats, BUBBLECHAIN_DTYPE, PoPhaseParams, PoPhaseInput, PoPhaseStats, ALIGNMENT_DTYPE, PoPhaseIndexStats, PoRelevantParams, PoRelevantInput, PoRelevantDims, PoRelevantStats, PoSpellInput, PoSpellStats
from .phasing import BubblePaths, RelevantReads
from .spelling import spell_arrays

OverlapT = Tuple[str, str, int, int, int, int]

_PYT = [False, None]


def _pytuples():
    """``po_rows_to_tuples`` of phasm_amd/_pytuples.so (built by phasm_amd.build.build_pytuples), or None."""
    if not _PYT[0]:
        _PYT[0] = True
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_pytuples.so")
        if os.path.exists(path) and not os.environ.get("PHASM_NO_PYTUPLES"):
            try:
                lib = ctypes.PyDLL(path)
                lib.po_rows_to_tuples.restype = ctypes.py_object
                lib.po_rows_to_tuples.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.py_object]
                _PYT[1] = lib.po_rows_to_tuples
            except (OSError, AttributeError):
                _PYT[1] = None
    return _PYT[1]


def _to_bytes(x, what: str) -> bytes:
    if isinstance(x, bytes):
        return x
    if isinstance(x, str):
        return x.encode("utf-8")
    if isinstance(x, (bytearray, memoryview)):
        return bytes(x)
    raise TypeError("%s must be str or bytes, not %s" % (what, type(x).__name__))


def _check(handle, status: int):
    if status == _lib.PO_OK:
        return
    msg = _lib.load().po_last_error(handle)
    msg = msg.decode("utf-8", "replace") if msg else "libphasm_overlap error %d" % status
    if status == _lib.PO_ERR_NOMEM:
        raise MemoryError(msg)
    if status == _lib.PO_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def _ptr(a: np.ndarray):
    """The address of an array's data for a C call; NULL for an empty array."""
    return a.ctypes.data_as(ctypes.c_void_p) if len(a) else None


class DeviceWalk:
    """Owns one walk (``po_walk_create``): the candidate sets of ``BubbleChainPhaser`` on the device.  The interface of
    ``phasm_amd.phasing.HostWalk``."""

    def __init__(self, owner: "ExactOverlapper", ploidy: int):
        if not 0 <= int(ploidy) < 2**32:
            raise ValueError("po_walk_create: the ploidy must be 1 to 8")
        self._owner, self._lib = owner, _lib.load()
        self._ptr = ctypes.c_void_p()
        _check(owner._h, self._lib.po_walk_create(owner._h, int(ploidy), ctypes.byref(self._ptr)))
        self.ploidy = int(ploidy)

    def _call(self, status: int):
        _check(self._owner._h, status)

    def info(self) -> dict:
        out = _lib.PoWalkInfo()
        self._call(self._lib.po_walk_info_get(self._ptr, ctypes.byref(out)))
        return out.as_dict()

    @property
    def start_of_block(self) -> bool:
        return bool(self.info()["start_of_block"])

    def reset(self) -> None:
        self._call(self._lib.po_walk_reset(self._ptr))

    def phase_stats(self) -> dict:
        return self._owner.phase_stats()

    def walk_stats(self) -> dict:
        return self._owner.walk_stats()

    def step(self, rel, path_reads, start_of_block, threshold: float = 0.0, min_spanning_reads: int = 0, levels=None,
             max_candidates: int = 0, advance: bool = True, cap: Optional[int] = None):
        """``po_walk_step``: ``po_phase_branch`` on the bubble whose read sets are the walk's.  ``rel``: the
        ``RelevantReads`` of the bubble; ``path_reads[p]``: the interior reads of path p as global ids (MergedReads
        expanded).  The other arguments and the result ``(cand, ext, rl)`` are those of ``ExactOverlapper.phase_branch``.
        ``advance``: the final list becomes the walk's candidates (where it has an entry)."""
        from .phasing import walk_paths
        if not 0 <= int(min_spanning_reads) < 2**32 or not 0 <= int(max_candidates) < 2**32:
            raise ValueError("min_spanning_reads and max_candidates must fit 32 bits")
        path_off, path_ids = walk_paths(rel, path_reads)
        lv = np.ascontiguousarray(levels if levels is not None else [], dtype=np.float64)
        arrays = [np.ascontiguousarray(a, dtype=dt) for a, dt in (
            (rel.overlap_max, np.int32), (rel.aln_off, np.uint32), (rel.aln_b, np.uint32), (rel.aln_a0, np.int32), (rel.aln_a1, np.int32),
            (path_off, np.uint32), (path_ids, np.uint32))]
        R, P = len(rel.rel_reads), len(path_off) - 1
        if len(arrays[0]) != R or len(arrays[1]) != R + 1 or len({len(arrays[2]), len(arrays[3]), len(arrays[4])}) != 1 or \
                (R and len(arrays[2]) != int(arrays[1][-1])):
            raise ValueError("the arrays of the relevant reads do not have the lengths their sizes and offsets give")
        b_reads = np.ascontiguousarray(rel.b_reads, dtype=np.uint32)
        n_cands = self.info()["n_cands"]
        prm = PoPhaseParams(self.ploidy, P, n_cands, R, len(b_reads), int(bool(start_of_block)), int(min_spanning_reads),
                            int(levels is not None), int(max_candidates), len(lv), float(threshold), 0, 0)
        as_p = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
        inp = PoPhaseInput(*[as_p(a) for a in arrays], None, None, as_p(lv))
        if n_cands * P ** self.ploidy >= 2**31:
            raise ValueError("po_walk_step: too many extensions for one call")
        call = lambda adv, c, e, r, room: self._call(self._lib.po_walk_step(   # noqa: E731
            self._owner._h, self._ptr, ctypes.byref(prm), ctypes.byref(inp), _ptr(b_reads), int(bool(adv)), _ptr(c), _ptr(e), _ptr(r), room,
            ctypes.byref(n)))
        n = ctypes.c_uint64()
        none = np.zeros(0, dtype=np.uint32)
        room = n_cands * P ** self.ploidy if cap is None else int(cap)
        if cap is None and room > 1 << 22:
            call(False, none, none, none.astype(np.float64), 0)   # (a peek for the count: the step itself may run only once)
            room = int(n.value)
        cand, ext, rl = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.float64)
        call(advance, cand, ext, rl, room)
        m = min(room, int(n.value))
        return cand[:m].copy(), ext[:m].copy(), rl[:m].copy()

    def relevant(self, source, index, cur_graph, preds=(), start_of_block: bool = False, min_spanning_reads: int = 0,
                 without_prev_graph: bool = False) -> "ResidentRelevant":
        """``po_walk_relevant``: the gather of ``phase_relevant`` with ``prev_graph`` and ``prev_aligning`` taken from the walk,
        its arrays staying on the device for ``step_resident``.  ``source`` is the walk's own overlapper (given for the
        interface of ``HostWalk``); ``without_prev_graph``: ``prev_graph`` counts as empty (a large bubble)."""
        if source is not None and source is not self._owner:
            raise ValueError("po_walk_relevant: the walk belongs to another handle")
        if not 0 <= int(min_spanning_reads) < 2**32:
            raise ValueError("min_spanning_reads must fit 32 bits")
        preds = list(preds)
        cur = np.ascontiguousarray(list(cur_graph), dtype=np.uint32)
        pred = np.ascontiguousarray([p[0] for p in preds], dtype=np.uint32)
        plen = np.ascontiguousarray([p[1] for p in preds], dtype=np.int32)
        as_p = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
        prm = _lib.PoWalkRelevantParams(int(bool(start_of_block)), int(min_spanning_reads), int(bool(without_prev_graph)), 0)
        inp = PoRelevantInput(as_p(cur), len(cur), None, 0, None, 0, as_p(pred), as_p(plen), len(plen))
        r = ctypes.c_void_p()
        self._call(self._lib.po_walk_relevant(self._owner._h, self._ptr, index._ptr, ctypes.byref(prm), ctypes.byref(inp), ctypes.byref(r)))
        return ResidentRelevant(self, r)

    def step_resident(self, rel: "ResidentRelevant", path_reads, start_of_block, threshold: float = 0.0, min_spanning_reads: int = 0,
                      levels=None, max_candidates: int = 0, advance: bool = True, cap: Optional[int] = None):
        """``po_walk_step_resident``: ``step`` on the gather ``rel`` of ``relevant``, with nothing but the path reads (global
        ids) going up.  The arguments and the result are those of ``step``."""
        if not 0 <= int(min_spanning_reads) < 2**32 or not 0 <= int(max_candidates) < 2**32:
            raise ValueError("min_spanning_reads and max_candidates must fit 32 bits")
        lens = np.fromiter((len(p) for p in path_reads), dtype=np.int64, count=len(path_reads))
        path_off = np.zeros(len(lens) + 1, dtype=np.uint32)
        path_off[1:] = np.cumsum(lens)
        path_ids = np.ascontiguousarray([r for p in path_reads for r in p], dtype=np.uint32)
        lv = np.ascontiguousarray(levels if levels is not None else [], dtype=np.float64)
        P, n_cands = len(lens), self.info()["n_cands"]
        prm = PoPhaseParams(self.ploidy, P, n_cands, rel.n_relevant, rel.n_b, int(bool(start_of_block)), int(min_spanning_reads),
                            int(levels is not None), int(max_candidates), len(lv), float(threshold), 0, 0)
        as_p = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
        inp = PoPhaseInput(None, None, None, None, None, path_off.ctypes.data, as_p(path_ids), None, None, as_p(lv))
        if n_cands * max(P, 1) ** self.ploidy >= 2**31:
            raise ValueError("po_walk_step_resident: too many extensions for one call")
        n = ctypes.c_uint64()
        call = lambda adv, c, e, r, room: self._call(self._lib.po_walk_step_resident(   # noqa: E731
            self._owner._h, self._ptr, rel._ptr, ctypes.byref(prm), ctypes.byref(inp), int(bool(adv)), _ptr(c), _ptr(e), _ptr(r), room,
            ctypes.byref(n)))
        none = np.zeros(0, dtype=np.uint32)
        room = n_cands * P ** self.ploidy if cap is None else int(cap)
        if cap is None and room > 1 << 22:
            call(False, none, none, none.astype(np.float64), 0)   # (a peek for the count: the step itself may run only once)
            room = int(n.value)
        cand, ext, rl = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.float64)
        call(advance, cand, ext, rl, room)
        m = min(room, int(n.value))
        return cand[:m].copy(), ext[:m].copy(), rl[:m].copy()

    def prev_sets(self):
        """``po_walk_prev_copy``: ``(prev_graph, prev_aligning)`` as ascending lists of global read ids."""
        out = []
        for which in (0, 1):
            n = ctypes.c_uint64()
            self._call(self._lib.po_walk_prev_copy(self._ptr, which, None, 0, ctypes.byref(n)))
            ids = np.zeros(int(n.value), dtype=np.uint32)
            if len(ids):
                self._call(self._lib.po_walk_prev_copy(self._ptr, which, ids.ctypes.data, len(ids), ctypes.byref(n)))
            out.append(ids.tolist())
        return out[0], out[1]

    def best(self):
        """``po_walk_best``: ``prune(candidate_sets, 1.0)`` -- ``(candidates, greatest log_rl)``."""
        room = self.info()["n_cands"]
        out = np.zeros(room, dtype=np.uint32)
        n, top = ctypes.c_uint64(), ctypes.c_double()
        self._call(self._lib.po_walk_best(self._ptr, _ptr(out), room, ctypes.byref(n), ctypes.byref(top)))
        return out[:int(n.value)].tolist(), float(top.value)

    def history(self, cands) -> np.ndarray:
        """``po_walk_history``: the extension id of each named candidate at every advanced bubble of the block, oldest first."""
        cands = np.ascontiguousarray(list(cands), dtype=np.uint32)
        depth = self.info()["depth"]
        out = np.zeros((len(cands), depth), dtype=np.uint32)
        self._call(self._lib.po_walk_history(self._ptr, _ptr(cands), len(cands), out.ctypes.data if out.size else None))
        return out

    def read_sets(self, cands) -> list:
        """``po_walk_read_sets``: the k read sets of each named candidate as ascending lists of global read ids."""
        cands = np.ascontiguousarray(list(cands), dtype=np.uint32)
        off = np.zeros(len(cands) * self.ploidy + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        self._call(self._lib.po_walk_read_sets(self._ptr, _ptr(cands), len(cands), off.ctypes.data, None, 0, ctypes.byref(n)))
        ids = np.zeros(int(n.value), dtype=np.uint32)
        if len(ids):
            self._call(self._lib.po_walk_read_sets(self._ptr, _ptr(cands), len(cands), off.ctypes.data, ids.ctypes.data, len(ids), ctypes.byref(n)))
        off, k = off.tolist(), self.ploidy
        return [[ids[off[q * k + i]:off[q * k + i + 1]].tolist() for i in range(k)] for q in range(len(cands))]

    def close(self) -> None:
        if getattr(self, "_ptr", None):
            self._lib.po_result_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            if self._owner._h:
                self.close()
        except Exception:
            pass


class ResidentRelevant:
    """The gather of ``DeviceWalk.relevant`` (``po_walk_relevant``): its sizes as attributes; the arrays stay on the device until
    ``fetch()`` asks for them.  It is live until the walk's next ``relevant``, a ``reset`` or the walk's ``close``."""

    def __init__(self, walk: DeviceWalk, ptr):
        self._walk, self._lib, self._ptr = walk, walk._lib, ptr
        d = PoRelevantDims()
        try:
            walk._call(self._lib.po_relevant_sizes(ptr, ctypes.byref(d)))
        except Exception:
            self.close()
            raise
        self.n_cur_aligning, self.n_spanning, self.n_relevant = int(d.n_cur_aligning), int(d.n_spanning), int(d.n_relevant)
        self.n_alignments, self.n_b, self.fell_back = int(d.n_alignments), int(d.n_b), bool(d.fell_back)

    def fetch(self) -> "RelevantReads":
        """``po_relevant_copy``: what ``phase_relevant`` returns for the same sets passed as lists."""
        R, A = self.n_relevant, self.n_alignments
        out = RelevantReads(np.zeros(self.n_cur_aligning, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.int32), np.zeros(R + 1, np.uint32),
                            np.zeros(A, np.uint32), np.zeros(A, np.int32), np.zeros(A, np.int32), np.zeros(self.n_b, np.uint32),
                            self.n_spanning, self.fell_back)
        self._walk._call(self._lib.po_relevant_copy(self._ptr, _ptr(out.cur_aligning), _ptr(out.rel_reads), _ptr(out.overlap_max),
                                                    _ptr(out.aln_off), _ptr(out.aln_b), _ptr(out.aln_a0), _ptr(out.aln_a1), _ptr(out.b_reads)))
        return out

    def close(self) -> None:
        if getattr(self, "_ptr", None):
            self._lib.po_result_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            if self._walk._owner._h:
                self.close()
        except Exception:
            pass


class DevicePaths(BubblePaths):
    """Owns a ``po_phase_paths`` result that STAYS on the device (``ExactOverlapper.phase_paths_resident``).  The bubble-sized
    arrays -- table, interiors, exit predecessors, ``bubble_path_off`` -- come home once; the listed paths do not:
    ``paths_of(b)`` and ``path_of(b, p)`` fetch a range through ``po_paths_copy_paths``, ``score_large`` scores every listed
    path of a bubble where it is (``po_phase_large``).  The accessors are those of ``phasm_amd.phasing.BubblePaths``
    (``path_off`` and ``path_nodes`` stay empty).  ``close()`` frees the device result (and whatever ``owned`` names, in
    order: the handle of a graph that lives only for these paths); the graph it was listed from may be freed before."""

    def __init__(self, owner: "ExactOverlapper", ptr, owned=()):
        self._owner, self._lib, self._ptr, self._owned = owner, _lib.load(), ptr, list(owned)
        try:
            d = _lib.PoPathsDims()
            _check(owner._h, self._lib.po_paths_sizes(ptr, ctypes.byref(d)))
            nb = int(d.n_bubbles)
            super().__init__(np.zeros(nb, _lib.BUBBLE_PATHS_DTYPE), np.zeros(nb + 1, np.uint64), np.zeros(int(d.n_inside_nodes), np.uint32),
                             np.zeros(nb + 1, np.uint64), np.zeros(int(d.n_preds), np.uint32), np.zeros(int(d.n_preds), np.int32),
                             np.zeros(nb + 1, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
            self.n_listed_paths, self.n_path_nodes = int(d.n_listed_paths), int(d.n_path_nodes)
            _check(owner._h, self._lib.po_paths_copy(ptr, _ptr(self.bubbles), _ptr(self.inside_off), _ptr(self.inside_nodes), _ptr(self.pred_off),
                                                     _ptr(self.pred_node), _ptr(self.pred_weight), _ptr(self.bubble_path_off), None, None))
        except Exception:
            self.close()
            raise

    def _range(self, first: int, count: int):
        """``(offsets relative to the first path, nodes)`` of the listed paths first .. first + count - 1."""
        if self._ptr is None:
            raise ValueError("the device paths are closed")
        off, n = np.zeros(count + 1, dtype=np.uint64), ctypes.c_uint64()
        _check(self._owner._h, self._lib.po_paths_copy_paths(self._ptr, int(first), int(count), _ptr(off), None, 0, ctypes.byref(n)))
        nodes = np.zeros(int(n.value), dtype=np.uint32)
        _check(self._owner._h, self._lib.po_paths_copy_paths(self._ptr, int(first), int(count), None, _ptr(nodes), len(nodes), ctypes.byref(n)))
        return off, nodes

    def paths_of(self, b: int) -> List[tuple]:
        """``BubblePaths.paths_of``, fetched from the device when asked."""
        if not self.is_listed(b):
            return super().paths_of(b)   # (raises: the paths were not listed)
        first, last = int(self.bubble_path_off[b]), int(self.bubble_path_off[b + 1])
        off, nodes = self._range(first, last - first)
        return [tuple(nodes[int(off[p]):int(off[p + 1])].tolist()) for p in range(last - first)]

    def path_of(self, b: int, p: int) -> tuple:
        """Listed path ``p`` (0-based within bubble b) alone, both ends included."""
        first, n = int(self.bubble_path_off[b]), int(self.bubble_path_off[b + 1]) - int(self.bubble_path_off[b])
        if not self.is_listed(b) or not 0 <= int(p) < n:
            raise ValueError("bubble %d has no listed path %d" % (b, p))
        return tuple(self._range(first + int(p), 1)[1].tolist())

    def score_large(self, b: int, rel: "RelevantReads", reads_of_node, n_best: int, want_scores: bool = False):
        """``po_phase_large`` on bubble b: ``(best, best_scores, scores or None)`` -- the ``n_best`` best path indices within the
        bubble as ``sorted(range(P), key=score.get, reverse=True)[:n_best]`` gives them, their scores, and with
        ``want_scores`` the score of every listed path.  ``rel``: the relevant reads (``phasing.relevant_reads``);
        ``reads_of_node(node)``: the read ids of a node."""
        from .phasing import large_node_lists
        if self._ptr is None:
            raise ValueError("the device paths are closed")
        if not 0 <= int(b) < len(self) or not 0 <= int(n_best) < 2**32:
            raise ValueError("po_phase_large: bubble %d is not below the %d bubbles of the result" % (b, len(self)))
        R = len(rel.rel_reads)
        if R == 0:
            raise ZeroDivisionError("no relevant reads")
        node_off, node_ids = large_node_lists(rel, self.interior_of(b), reads_of_node)
        arrays = [np.ascontiguousarray(a, dtype=dt) for a, dt in (
            (rel.overlap_max, np.int32), (rel.aln_off, np.uint32), (rel.aln_b, np.uint32), (rel.aln_a0, np.int32), (rel.aln_a1, np.int32),
            (node_off, np.uint32), (node_ids, np.uint32))]
        if len(arrays[0]) != R or len(arrays[1]) != R + 1 or len({len(arrays[2]), len(arrays[3]), len(arrays[4])}) != 1 or \
                len(arrays[2]) != int(arrays[1][-1]):
            raise ValueError("the arrays of the relevant reads do not have the lengths their offsets give")
        prm = _lib.PoLargeParams(int(b), R, len(rel.b_reads), int(n_best), 0)
        inp = _lib.PoLargeInput(*[a.ctypes.data if len(a) else None for a in arrays], len(node_off) - 1)
        n_paths = int(self.bubble_path_off[b + 1]) - int(self.bubble_path_off[b])
        best, best_scores = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.float64)
        scores = np.zeros(n_paths if want_scores else 0, dtype=np.float64)
        n = ctypes.c_uint32()
        _check(self._owner._h, self._lib.po_phase_large(self._owner._h, self._ptr, ctypes.byref(prm), ctypes.byref(inp), _ptr(best),
                                                        _ptr(best_scores), _ptr(scores), ctypes.byref(n)))
        k = int(n.value)
        return [int(x) for x in best[:k]], best_scores[:k].copy(), (scores if want_scores else None)

    def large_stats(self) -> dict:
        return self._owner.large_stats()

    def close(self) -> None:
        if getattr(self, "_ptr", None) is not None:
            self._lib.po_result_free(self._ptr)
            self._ptr = None
        while getattr(self, "_owned", None):
            self._owned.pop(0).close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OverlapResult:
    """Owns one ``po_result``: rows stay on the device until asked for."""

    def __init__(self, owner: "ExactOverlapper", ptr, dtype=ROW_DTYPE):
        self._owner = owner
        self._ptr = ptr
        self._dtype = dtype  # ROW_DTYPE (24-byte rows) or CAND_DTYPE (16-byte verified candidates)
        self._lib = _lib.load()

    def __len__(self) -> int:
        return int(self._lib.po_result_count(self._ptr)) if self._ptr else 0

    def rows(self) -> np.ndarray:
        """Host copy as a structured array (a_idx, b_idx, astart, aend, bstart, bend)."""
        n = len(self)
        if n == 0:
            return np.empty(0, dtype=self._dtype)
        p = self._lib.po_result_rows(self._ptr)
        if not p:
            _check(self._owner._h, _lib.PO_ERR_HIP)
        buf = (ctypes.c_char * (n * self._dtype.itemsize)).from_address(p)
        return np.frombuffer(buf, dtype=self._dtype).copy()

    def rows_view(self) -> np.ndarray:
        """The same rows WITHOUT the copy: a read-only view of the library's page-locked host buffer, valid until
        ``free()`` (the C ABI's ``po_result_rows`` pointer as it is)."""
        n = len(self)
        if n == 0:
            return np.empty(0, dtype=self._dtype)
        p = self._lib.po_result_rows(self._ptr)
        if not p:
            _check(self._owner._h, _lib.PO_ERR_HIP)
        buf = (ctypes.c_char * (n * self._dtype.itemsize)).from_address(p)
        v = np.frombuffer(buf, dtype=self._dtype)
        v.flags.writeable = False
        return v

    def rows_range_view(self, first: int, count: int) -> np.ndarray:
        """``po_result_rows_range``: rows [first, first + count) in page-locked host memory (a view, valid until the
        next call on the overlapper) -- one rank's share of a merged multi-GPU result."""
        if count <= 0:
            return np.empty(0, dtype=self._dtype)
        p = self._lib.po_result_rows_range(self._ptr, int(first), int(count))
        if not p:
            _check(self._owner._h, _lib.PO_ERR_HIP)
        buf = (ctypes.c_char * (count * self._dtype.itemsize)).from_address(p)
        v = np.frombuffer(buf, dtype=self._dtype)
        v.flags.writeable = False
        return v

    def write_gfa_edges(self, fileobj) -> int:
        """Native bulk writer of the GFA2 ``E`` lines (``po_write_gfa_edges``) to a real file."""
        fileobj.flush()
        n = ctypes.c_uint64()
        _check(self._owner._h, self._lib.po_write_gfa_edges(self._ptr, fileobj.fileno(), ctypes.byref(n)))
        return int(n.value)

    def device_ptr(self) -> int:
        return int(self._lib.po_result_device_rows(self._ptr) or 0)

    def node_order(self) -> np.ndarray:
        """``po_result_node_order``: the nodes of an edge result's graph in the order the reference's graph holds
        them (``for n in g``), which tip removal follows."""
        n = ctypes.c_uint64()
        _check(self._owner._h, self._lib.po_result_node_order(self._ptr, None, 0, ctypes.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint32)
        if len(out):
            _check(self._owner._h, self._lib.po_result_node_order(self._ptr, out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(n)))
        return out

    def merged_paths(self):
        """``po_result_merged_paths`` of a ``layout_merge`` result: ``(offsets, members, prefix_lengths, lengths)`` --
        merged node k (node id ``len(owner) + k``) holds the reads ``members[offsets[k]:offsets[k + 1]]`` in path order,
        ``prefix_lengths`` has the weight of the link out of each member (0 for a path's last) and ``lengths[k]`` is the
        merged node's length."""
        k, m = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._owner._h, self._lib.po_result_merged_paths(self._ptr, ctypes.byref(k), ctypes.byref(m), None, 0, None, None, 0, None))
        offsets = np.zeros(int(k.value) + 1, dtype=np.uint64)
        lengths = np.zeros(int(k.value), dtype=np.int64)
        members = np.zeros(int(m.value), dtype=np.uint32)
        prefix = np.zeros(int(m.value), dtype=np.int32)
        _check(self._owner._h, self._lib.po_result_merged_paths(self._ptr, ctypes.byref(k), ctypes.byref(m), _ptr(offsets), len(lengths),
                                                                 _ptr(members), _ptr(prefix), len(members), _ptr(lengths)))
        return offsets, members, prefix, lengths

    def copy_to_device(self, dst_ptr: int, count: Optional[int] = None) -> None:
        """Device-to-device copy of the first ``count`` entries (default: all) to ``dst_ptr``."""
        if count is None or count >= len(self):
            _check(self._owner._h, self._lib.po_result_copy_to_device(self._ptr, ctypes.c_void_p(dst_ptr)))
        elif count > 0:
            _check(self._owner._h, self._lib.po_result_copy_prefix_to_device(self._ptr, ctypes.c_void_p(dst_ptr), int(count)))

    def free(self) -> None:
        if self._ptr and self._owner._h:
            self._lib.po_result_free(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ExactOverlapper:
    def __init__(self, device: Optional[int] = None):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        st = self._lib.po_create(ctypes.byref(h))
        if st != _lib.PO_OK:
            raise MemoryError("po_create failed")
        self._h = h
        self._results: List[OverlapResult] = []
        if device is not None:
            _check(self._h, self._lib.po_set_device(self._h, int(device)))

    # ---- the reference API -------------------------------------------------------------
    def add_sequence(self, id, seq) -> None:
        bid = _to_bytes(id, "id")
        bseq = _to_bytes(seq, "seq")
        _check(self._h, self._lib.po_add_sequence(self._h, bid, len(bid), bseq, len(bseq)))

    def add_sequence_ptr(self, id, address: int, length: int) -> None:
        """``po_add_sequence`` as the C ABI has it: the sequence is ``length`` bytes at ``address`` (copied, like every
        sequence: the caller's memory is never written -- the GPU tests hand in a read-only mapping to hold the library
        to that, tests/checker.py GuardedReads)."""
        bid = _to_bytes(id, "id")
        _check(self._h, self._lib.po_add_sequence(self._h, bid, len(bid), ctypes.c_char_p(int(address)), int(length)))

    def add_fasta(self, path: str, both_strands: bool = True) -> int:
        """Native FASTA ingest (``po_add_fasta``): every record as ``name+`` / sequence and ``name-`` /
        reverse complement, as ``phasm overlap`` adds them (assembler.py:38-40).  Returns the record count."""
        n = ctypes.c_uint64()
        _check(self._h, self._lib.po_add_fasta(self._h, os.fsencode(path), 1 if both_strands else 0, ctypes.byref(n)))
        return int(n.value)

    def write_gfa_segments(self, fileobj) -> int:
        """``S <name> <length> *`` for every read pair, written natively to a real file (``po_write_gfa_segments``)."""
        fileobj.flush()
        n = ctypes.c_uint64()
        _check(self._h, self._lib.po_write_gfa_segments(self._h, fileobj.fileno(), ctypes.byref(n)))
        return int(n.value)

    def overlaps(self, min_length: int) -> List[OverlapT]:
        res = self.overlaps_to_host_result(min_length)
        try:
            ids = self.ids()
            fn = _pytuples()
            if fn is not None and len(res):
                # the list of tuples built natively from the page-locked row array (phasm_amd/csrc/pytuples.c), as
                # pybind11 builds the reference's from std::vector<OverlapT> (src/phasm.cpp:15)
                p = self._lib.po_result_rows(res._ptr)
                if not p:   # (a failed device->host copy or page-locked allocation: raise, never hand NULL to the builder)
                    _check(self._h, _lib.PO_ERR_HIP)
                return fn(p, len(res), ids)
            arr = res.rows_view()
            a_ids = [ids[i] for i in arr["a_idx"].tolist()]
            b_ids = [ids[i] for i in arr["b_idx"].tolist()]
            return list(zip(a_ids, b_ids, arr["astart"].tolist(), arr["aend"].tolist(),
                            arr["bstart"].tolist(), arr["bend"].tolist()))
        finally:
            res.free()

    # ---- bulk / multi-GPU extensions ------------------------------------------------------
    @staticmethod
    def _min_length(min_length) -> int:
        if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)):
            raise TypeError("overlaps(): incompatible function arguments: min_length must be an unsigned int")
        if min_length < 0 or min_length > 0xFFFFFFFF:
            raise TypeError("overlaps(): incompatible function arguments: min_length must be an unsigned int")
        return int(min_length)

    def overlaps_result(self, min_length: int, shard: int = 0, nshards: int = 1) -> OverlapResult:
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_overlaps_shard(self._h, m, int(shard), int(nshards), ctypes.byref(r)))
        return OverlapResult(self, r)

    def overlaps_to_host_result(self, min_length: int) -> OverlapResult:
        """``po_overlaps_to_host``: the rows land in page-locked host memory while later chunks are still being
        computed; ``rows_view()`` / ``rows()`` of the result cost no further copy from the device."""
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_overlaps_to_host(self._h, m, ctypes.byref(r)))
        return OverlapResult(self, r)

    def overlaps_ex_result(self, min_length: int, max_diff: int = 0, band: int = 0) -> OverlapResult:
        """``po_overlaps_ex``: banded seed-extension DP with up to ``max_diff`` differences (an extension beyond the
        exact reference; ``max_diff = 0`` gives the rows of ``overlaps``)."""
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_overlaps_ex(self._h, m, int(max_diff), int(band), ctypes.byref(r)))
        return OverlapResult(self, r)

    def overlaps_ex_array(self, min_length: int, max_diff: int = 0, band: int = 0) -> np.ndarray:
        res = self.overlaps_ex_result(min_length, max_diff, band)
        try:
            return res.rows()
        finally:
            res.free()

    def candidates_result(self, min_length: int, shard: int = 0, nshards: int = 1) -> OverlapResult:
        """Verified candidates of one a-side shard (``po_candidates_shard``): the compact form that
        travels between GPUs; ``expand_result`` turns the merged array into rows."""
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_candidates_shard(self._h, m, int(shard), int(nshards), ctypes.byref(r)))
        return OverlapResult(self, r, CAND_DTYPE)

    def candidates_result_into(self, min_length: int, shard: int, nshards: int, dst_ptr: int, capacity: int):
        """``po_candidates_shard_into``: (result, written) -- the candidates go straight to ``dst_ptr`` when they fit."""
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        w = ctypes.c_int()
        _check(self._h, self._lib.po_candidates_shard_into(self._h, m, int(shard), int(nshards), ctypes.c_void_p(dst_ptr),
                                                           int(capacity), ctypes.byref(w), ctypes.byref(r)))
        return OverlapResult(self, r, CAND_DTYPE), bool(w.value)

    # ---- sliced wide index (multi-GPU; phasm_amd/dist.py IndexExchange) -----------------------------------
    def index_slice_build(self, min_length: int, slice_: int, n_slices: int) -> Tuple[bool, int, int]:
        """``po_index_slice_build``: build sub-table ``slice_`` of ``n_slices``; (is_wide, slice_bits, chain_entries)."""
        m = self._min_length(min_length)
        w, b, e = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        _check(self._h, self._lib.po_index_slice_build(self._h, m, int(slice_), int(n_slices), ctypes.byref(w), ctypes.byref(b), ctypes.byref(e)))
        return bool(w.value), int(b.value), int(e.value)

    def index_chunk_bytes(self, slice_bits: int, chain_capacity: int) -> int:
        return int(self._lib.po_index_chunk_bytes(int(slice_bits), int(chain_capacity), None))

    def index_slice_export(self, dst_ptr: int, chain_capacity: int) -> None:
        _check(self._h, self._lib.po_index_slice_export(self._h, ctypes.c_void_p(dst_ptr), int(chain_capacity)))

    def candidates_result_indexed(self, min_length: int, shard: int, nshards: int, index_ptr: int, n_slices: int, slice_bits: int,
                                  chain_capacity: int, dst_ptr: int = 0, capacity: int = 0):
        """``po_candidates_shard_indexed``: the shard call on a gathered sliced index; (result, written)."""
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        w = ctypes.c_int()
        _check(self._h, self._lib.po_candidates_shard_indexed(self._h, m, int(shard), int(nshards), ctypes.c_void_p(index_ptr),
                                                              int(n_slices), int(slice_bits), int(chain_capacity),
                                                              ctypes.c_void_p(dst_ptr) if dst_ptr else None, int(capacity),
                                                              ctypes.byref(w), ctypes.byref(r)))
        return OverlapResult(self, r, CAND_DTYPE), bool(w.value)

    def overlaps_shard_indexed_array(self, min_length: int, shard: int, nshards: int, index_ptr: int, n_slices: int,
                                     slice_bits: int, chain_capacity: int) -> np.ndarray:
        m = self._min_length(min_length)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_overlaps_shard_indexed(self._h, m, int(shard), int(nshards), ctypes.c_void_p(index_ptr),
                                                            int(n_slices), int(slice_bits), int(chain_capacity), ctypes.byref(r)))
        res = OverlapResult(self, r)
        try:
            return res.rows()
        finally:
            res.free()

    def expand_result(self, cand_device_ptr: int, n_candidates: int) -> OverlapResult:
        """Rows from a candidate array resident on this handle's device (``po_expand``)."""
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_expand(self._h, ctypes.c_void_p(cand_device_ptr), int(n_candidates), ctypes.byref(r)))
        return OverlapResult(self, r)

    def overlaps_array(self, min_length: int) -> np.ndarray:
        res = self.overlaps_to_host_result(min_length)
        try:
            return res.rows()
        finally:
            res.free()

    def overlaps_shard_array(self, min_length: int, shard: int, nshards: int) -> np.ndarray:
        res = self.overlaps_result(min_length, shard, nshards)
        try:
            return res.rows()
        finally:
            res.free()

    def shard_range(self, shard: int, nshards: int) -> Tuple[int, int]:
        """Read-index range scanned on the a-side by shard ``shard`` of ``nshards`` (host logic)."""
        b, e = ctypes.c_uint32(), ctypes.c_uint32()
        _check(self._h, self._lib.po_shard_range(self._h, int(shard), int(nshards), ctypes.byref(b), ctypes.byref(e)))
        return b.value, e.value

    def upload(self) -> None:
        _check(self._h, self._lib.po_upload(self._h))

    def upload_piece(self, shard: int, nshards: int, dst_ptr: int = 0, capacity_words: int = 0) -> Tuple[bool, int]:
        """``po_upload_piece``: (ok, words of the piece); with ``dst_ptr`` the piece is copied host->device there."""
        n, ok = ctypes.c_uint64(), ctypes.c_int()
        _check(self._h, self._lib.po_upload_piece(self._h, int(shard), int(nshards), ctypes.c_void_p(dst_ptr) if dst_ptr else None,
                                                  int(capacity_words), ctypes.byref(n), ctypes.byref(ok)))
        return bool(ok.value), int(n.value)

    def upload_assemble(self, pieces_ptr: int, slot_words: int, nshards: int, nparts: int = 1) -> None:
        _check(self._h, self._lib.po_upload_assemble_parts(self._h, ctypes.c_void_p(pieces_ptr), int(slot_words), int(nshards), int(nparts)))

    def upload_piece_part(self, shard: int, nshards: int, part: int, nparts: int, dst_ptr: int = 0, capacity_words: int = 0) -> Tuple[bool, int]:
        """``po_upload_piece_part``: part ``part`` of ``nparts`` of shard ``shard``'s piece (see ``upload_piece``)."""
        n, ok = ctypes.c_uint64(), ctypes.c_int()
        _check(self._h, self._lib.po_upload_piece_part(self._h, int(shard), int(nshards), int(part), int(nparts),
                                                       ctypes.c_void_p(dst_ptr) if dst_ptr else None, int(capacity_words),
                                                       ctypes.byref(n), ctypes.byref(ok)))
        return bool(ok.value), int(n.value)

    def invalidate(self) -> None:
        """``po_invalidate``: the next upload / overlaps call copies the packed reads to the device again."""
        _check(self._h, self._lib.po_invalidate(self._h))

    # ---- the consumer side: stage 1 of `phasm layout` (phasm_amd/layout.py is the host mirror) ----
    def add_segment(self, name, length: int) -> None:
        """One GFA2 ``S`` line without sequence (``po_add_segment``): nodes ``name+`` and ``name-``."""
        b = _to_bytes(name, "name")
        _check(self._h, self._lib.po_add_segment(self._h, b, len(b), int(length)))

    def add_gfa(self, path: str) -> Tuple[int, OverlapResult]:
        """Read a GFA2 file into this (empty) handle: segments become sequence-less reads, ``E`` lines
        the returned row result (``po_add_gfa``).  Returns (segment count, rows)."""
        n = ctypes.c_uint64()
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_add_gfa(self._h, os.fsencode(path), ctypes.byref(n), ctypes.byref(r)))
        return int(n.value), OverlapResult(self, r)

    def result_from_rows(self, rows: np.ndarray) -> OverlapResult:
        """Wrap caller-supplied rows (structured ROW_DTYPE or int array [n, 6]) into a result."""
        if rows.dtype != ROW_DTYPE:
            arr = np.asarray(rows)
            out = np.empty(len(arr), dtype=ROW_DTYPE)
            for k, name in enumerate(ROW_DTYPE.names):
                out[name] = arr[:, k]
            rows = out
        rows = np.ascontiguousarray(rows)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_result_from_rows(self._h, rows.ctypes.data_as(ctypes.c_void_p), len(rows), ctypes.byref(r)))
        return OverlapResult(self, r)

    def layout_edges(self, rows: OverlapResult, min_read_length: int = 0, min_overlap_length: int = 0,
                     max_overhang_abs: int = 1000, max_overhang_rel: float = 0.8,
                     want_removed: bool = True) -> Tuple[OverlapResult, Optional[np.ndarray]]:
        """``po_layout_edges``: assembly-graph edges (EDGE_DTYPE result) and the contained-read flags."""
        prm = PoLayoutParams(int(min_read_length), int(min_overlap_length), int(max_overhang_abs), 0, float(max_overhang_rel))
        removed = np.zeros(len(self) // 2, dtype=np.uint8) if want_removed else None
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_layout_edges(
            self._h, rows._ptr, ctypes.byref(prm),
            removed.ctypes.data_as(ctypes.c_void_p) if removed is not None and len(removed) else None, ctypes.byref(r)))
        return OverlapResult(self, r, EDGE_DTYPE), removed

    def _edge_stage(self, fn, edges: OverlapResult, prm, want_flags: bool):
        """The tail of the stage-2 calls: ``fn(handle, edges, params, flags, &result)``; the kept edges (EDGE_DTYPE
        result), or with ``want_flags`` the pair (kept edges, one byte per input edge)."""
        flags = np.zeros(len(edges), dtype=np.uint8) if want_flags else None
        r = ctypes.c_void_p()
        _check(self._h, fn(self._h, edges._ptr, ctypes.byref(prm),
                           flags.ctypes.data_as(ctypes.c_void_p) if flags is not None and len(flags) else None, ctypes.byref(r)))
        kept = OverlapResult(self, r, EDGE_DTYPE)
        return (kept, flags) if want_flags else kept

    def _stats(self, fn, struct) -> dict:
        s = struct()
        _check(self._h, fn(self._h, ctypes.byref(s)))
        return s.as_dict()

    def layout_stats(self) -> dict:
        return self._stats(self._lib.po_get_layout_stats, PoLayoutStats)

    def layout_reduce(self, edges: OverlapResult, length_fuzz: int = 1000, want_flags: bool = False):
        """``po_layout_reduce``: transitive reduction (``remove_transitive_edges``) and ``make_symmetric`` on a
        ``layout_edges`` result, which stays valid.  Returns the kept edges (EDGE_DTYPE result), or with
        ``want_flags`` the pair (kept edges, one byte per input edge: 0 kept, 1 transitive, 2 asymmetric)."""
        if not -2**31 <= int(length_fuzz) < 2**31:
            raise ValueError("length_fuzz does not fit 32 bits")
        prm = PoReduceParams(int(length_fuzz), 0)
        return self._edge_stage(self._lib.po_layout_reduce, edges, prm, want_flags)

    def reduce_stats(self) -> dict:
        return self._stats(self._lib.po_get_reduce_stats, PoReduceStats)

    def layout_tips(self, edges: OverlapResult, max_tip_len: int = 4, max_tip_len_bases: int = 5000, want_flags: bool = False):
        """``po_layout_tips``: ``remove_tips`` + ``make_symmetric`` + ``clean_graph`` on an edge result (of
        ``layout_edges``, ``layout_reduce`` or this call), which stays valid.  Returns the kept edges (EDGE_DTYPE
        result), or with ``want_flags`` the pair (kept edges, one byte per input edge: 0 kept, 1 incoming-tip edge,
        2 outgoing-tip edge, 3 asymmetric)."""
        if not 0 <= int(max_tip_len) < 2**32:
            raise ValueError("max_tip_len does not fit 32 bits")
        if not -2**31 <= int(max_tip_len_bases) < 2**31:
            raise ValueError("max_tip_len_bases does not fit 32 bits")
        prm = PoTipsParams(int(max_tip_len), int(max_tip_len_bases), 0)
        return self._edge_stage(self._lib.po_layout_tips, edges, prm, want_flags)

    def layout_diamonds(self, edges: OverlapResult, want_flags: bool = False):
        """``po_layout_diamonds``: ``remove_diamond_tips`` on an edge result (of ``layout_edges``, ``layout_reduce``,
        ``layout_tips`` or this call), which stays valid.  Returns the kept edges (EDGE_DTYPE result), or with
        ``want_flags`` the pair (kept edges, one byte per input edge: 0 kept, 1 in-edge of a removed end node, 2 the
        in-edge of a removed pred1).  Nodes left without an edge stay in the result's node order."""
        prm = PoDiamondParams(0)
        return self._edge_stage(self._lib.po_layout_diamonds, edges, prm, want_flags)

    def diamond_stats(self) -> dict:
        return self._stats(self._lib.po_get_diamond_stats, PoDiamondStats)

    def layout_merge(self, edges: OverlapResult, want_flags: bool = False):
        """``po_layout_merge``: ``merge_unambiguous_paths`` on an edge result (of ``layout_edges``, ``layout_reduce``,
        ``layout_tips`` or ``layout_diamonds``), which stays valid.  Returns the merged graph (EDGE_DTYPE result: the
        kept edges in input order, merged node k written as ``len(self) + k``; ``merged_paths()`` and ``node_order()``
        describe its nodes), or with ``want_flags`` the pair (merged graph, one byte per input edge: 0 kept as it is,
        1 link of a path, 2 kept with a renamed end or a raised weight)."""
        prm = PoMergeParams(0)
        return self._edge_stage(self._lib.po_layout_merge, edges, prm, want_flags)

    def merge_stats(self) -> dict:
        return self._stats(self._lib.po_get_merge_stats, PoMergeStats)

    def layout_coverage(self, graph: OverlapResult, rows: OverlapResult) -> np.ndarray:
        """``po_layout_coverage``: the operands of the reference's ``average_coverage_path(g, read_alignments, [u, v])`` for
        every edge of ``graph`` (an edge result or a merged graph) from ALL the rows of ``rows`` (a row result); both stay
        valid.  Returns a structured array (``read_length_sum`` u8, ``path_length`` i8) in the graph's edge order; the
        reference's value is ``read_length_sum / path_length``."""
        prm = PoCoverageParams(0)
        out = np.zeros(len(graph), dtype=COVERAGE_DTYPE)
        _check(self._h, self._lib.po_layout_coverage(
            self._h, graph._ptr, rows._ptr, ctypes.byref(prm), out.ctypes.data_as(ctypes.c_void_p) if len(out) else None))
        return out

    def coverage_stats(self) -> dict:
        return self._stats(self._lib.po_get_coverage_stats, PoCoverageStats)

    def _graph_stage(self, fn, graph: OverlapResult, prm, n_order: Optional[int], outputs):
        """The analysis calls on a graph result: ``fn(handle, graph, params, *outputs, &count)``.  ``outputs`` lists
        (dtype, "node" | "edge") per array -- one entry per node of the order or per edge --, the last one the table, which
        is cut to the ``count`` entries the call filled."""
        if n_order is None:
            n_order = len(graph.node_order())
        arrays = [np.zeros(int(n_order) if per == "node" else len(graph), dtype=dt) for dt, per in outputs]
        n = ctypes.c_uint64()
        _check(self._h, fn(self._h, graph._ptr, ctypes.byref(prm), *[_ptr(a) for a in arrays], ctypes.byref(n)))
        return (*arrays[:-1], arrays[-1][:int(n.value)].copy())

    def layout_components(self, graph: OverlapResult, n_order: Optional[int] = None):
        """``po_layout_components``: the weakly connected components of a graph result (an edge result, a merged graph or a
        ``graph_from_edges`` result), which stays valid.  Returns ``(node_component, edge_component, table)``: the
        component of every node, parallel to ``graph.node_order()`` (``n_order``: its length, if the caller has it); the
        component of every edge in the graph's edge order; one entry (``first_node``, ``n_nodes``, ``n_edges``) per
        component.  Component i is the i-th in the order of each component's lowest-ranked node."""
        return self._graph_stage(self._lib.po_layout_components, graph, PoComponentsParams(0), n_order,
                                 [(np.uint32, "node"), (np.uint32, "edge"), (COMPONENT_DTYPE, "node")])

    def components_stats(self) -> dict:
        return self._stats(self._lib.po_get_components_stats, PoComponentsStats)

    def layout_partition(self, graph: OverlapResult, n_order: Optional[int] = None):
        """``po_layout_partition``: the strongly connected components of a graph result (of the kinds ``layout_components``
        takes), which stays valid, and what the reference's ``partition_graph`` (phasm/bubbles.py:32-84) makes of them.
        Returns ``(node_scc, node_flags, edge_class, table)``: the SCC and the ``PART_*`` flag byte of every node, parallel
        to ``graph.node_order()`` (``n_order``: its length, if the caller has it); the class byte of every edge in the
        graph's edge order; one entry (``first_node``, ``n_nodes``, ``n_edges``, ``n_r_in``, ``n_re_out``) per SCC.  SCC i
        is the i-th in the order of each SCC's lowest-ranked node."""
        return self._graph_stage(self._lib.po_layout_partition, graph, PoPartitionParams(0), n_order,
                                 [(np.uint32, "node"), (np.uint8, "node"), (np.uint8, "edge"), (SCC_DTYPE, "node")])

    def partition_stats(self) -> dict:
        return self._stats(self._lib.po_get_partition_stats, PoPartitionStats)

    def layout_superbubbles(self, graph: OverlapResult, n_order: Optional[int] = None):
        """``po_layout_superbubbles``: the superbubbles of the acyclic partitions of a graph result (of the kinds
        ``layout_components`` takes), which stays valid -- what the reference's ``SuperBubbleFinderDAG`` reports on every
        acyclic partition (phasm/bubbles.py:174-381, 411-414).  Returns ``(node_exit, node_inside, node_flags, table)``:
        per node, parallel to ``graph.node_order()`` (``n_order``: its length, if the caller has it), the exit of the
        superbubble it enters, the entrance of the innermost superbubble that holds it strictly (``NO_NODE`` where there is
        none) and the ``SB_*`` flag byte; one entry (``entrance``, ``exit``, ``n_inside``, ``nested``) per superbubble, in
        the order of the entrances' ranks."""
        return self._graph_stage(self._lib.po_layout_superbubbles, graph, PoSuperbubbleParams(0), n_order,
                                 [(np.uint32, "node"), (np.uint32, "node"), (np.uint8, "node"), (SUPERBUBBLE_DTYPE, "node")])

    def superbubble_stats(self) -> dict:
        return self._stats(self._lib.po_get_superbubble_stats, PoSuperbubbleStats)

    def layout_superbubbles_all(self, graph: OverlapResult, n_order: Optional[int] = None):
        """``po_layout_superbubbles_all``: the superbubbles of the whole graph, the cyclic partitions included, by root
        splitting.  ``graph`` stays valid and in HBM.  Returns what ``layout_superbubbles`` returns;
        on the nodes whose SCC is a singleton the entries are the same."""
        return self._graph_stage(self._lib.po_layout_superbubbles_all, graph, PoSuperbubbleAllParams(0), n_order,
                                 [(np.uint32, "node"), (np.uint32, "node"), (np.uint8, "node"), (SUPERBUBBLE_DTYPE, "node")])

    def superbubble_all_stats(self) -> dict:
        return self._stats(self._lib.po_get_superbubble_all_stats, PoSuperbubbleAllStats)

    def layout_bubblechains(self, graph: OverlapResult, min_nodes: int = 1, n_order: Optional[int] = None):
        """``po_layout_bubblechains``: the bubble chains of a graph result (of the kinds ``layout_components`` takes), which
        stays valid -- what the reference's ``build_bubblechains(component, min_nodes)`` yields on every component
        (phasm/assembly_graph.py:594-652).  Returns ``(node_chain, node_bubble, edge_chain, table)``: per node, parallel to
        ``graph.node_order()`` (``n_order``: its length, if the caller has it), its chain and the position in that chain of
        the top-level bubble that holds it (``NO_NODE`` where there is none); per edge, in the graph's edge order, the chain
        that holds both ends; one entry (``first_entrance``, ``last_exit``, ``n_bubbles``, ``n_nodes``, ``n_edges``) per
        chain, in the order of the heads' ranks."""
        if not 0 <= int(min_nodes) <= 0xFFFFFFFF:
            raise ValueError("min_nodes does not fit 32 bits")
        return self._graph_stage(self._lib.po_layout_bubblechains, graph, PoBubblechainParams(int(min_nodes), 0), n_order,
                                 [(np.uint32, "node"), (np.uint32, "node"), (np.uint32, "edge"), (BUBBLECHAIN_DTYPE, "node")])

    def bubblechain_stats(self) -> dict:
        return self._stats(self._lib.po_get_bubblechain_stats, PoBubblechainStats)

    def layout_bubblechains_all(self, graph: OverlapResult, min_nodes: int = 1, n_order: Optional[int] = None):
        """``po_layout_bubblechains_all``: ``layout_bubblechains`` behind the superbubbles of the whole graph
        (``layout_superbubbles_all``), the cyclic partitions included.  Returns what
        ``layout_bubblechains`` returns.  A RING CHAIN -- the top-level bubbles of a circular component, linked round -- holds
        all its bubbles; its head is the lowest-ranked entrance and ``last_exit == first_entrance`` marks it.  On a graph
        without a non-singleton SCC the arrays are byte-equal to ``layout_bubblechains``'."""
        if not 0 <= int(min_nodes) <= 0xFFFFFFFF:
            raise ValueError("min_nodes does not fit 32 bits")
        return self._graph_stage(self._lib.po_layout_bubblechains_all, graph, PoBubblechainParams(int(min_nodes), 0), n_order,
                                 [(np.uint32, "node"), (np.uint32, "node"), (np.uint32, "edge"), (BUBBLECHAIN_DTYPE, "node")])

    def bubblechain_all_stats(self) -> dict:
        return self._stats(self._lib.po_get_bubblechain_all_stats, PoBubblechainAllStats)

    def layout_contigs_all(self, graph: OverlapResult, min_contig_len: int = 5000, min_nodes: int = 1, exclude=None,
                           n_order: Optional[int] = None):
        """``po_layout_contigs_all``: ``layout_contigs`` with the chains of ``layout_bubblechains_all`` as the exclude set
        when ``exclude`` is None, ring chains included.  Arguments, result and stats (``contig_stats``) as ``layout_contigs``."""
        return self._contig_stage(self._lib.po_layout_contigs_all, graph, min_contig_len, min_nodes, exclude, n_order)

    def layout_contigs(self, graph: OverlapResult, min_contig_len: int = 5000, min_nodes: int = 1, exclude=None,
                       n_order: Optional[int] = None):
        """``po_layout_contigs``: the contigs of a graph result (of the kinds ``layout_components`` takes), which stays
        valid -- the paths and single nodes that the reference's ``identify_contigs(component, exclude_nodes, min_contig_len)``
        reports on every component (phasm/assembly_graph.py:655-718).  ``exclude`` None: the nodes of the bubble chains the
        call builds first (``min_nodes`` as in ``layout_bubblechains``), what `phasm chain` passes; else one byte per node,
        parallel to ``graph.node_order()`` (``n_order``: its length, if the caller has it), non-zero = excluded.  Returns
        ``(edge_contig, edge_pos, table)``: per edge, in the graph's edge order, its contig and its 0-based place on that
        contig's path (``NO_NODE`` where there is none); one entry (``first_node``, ``last_node``, ``n_nodes``,
        ``first_edge``, ``length``) per contig: the paths by (rank of the first node, head edge), then the one-node contigs
        by rank."""
        return self._contig_stage(self._lib.po_layout_contigs, graph, min_contig_len, min_nodes, exclude, n_order)

    def _contig_stage(self, fn, graph: OverlapResult, min_contig_len: int, min_nodes: int, exclude, n_order: Optional[int]):
        if not 0 <= int(min_nodes) <= 0xFFFFFFFF:
            raise ValueError("min_nodes does not fit 32 bits")
        if not 0 <= int(min_contig_len) < 2**64:
            raise ValueError("min_contig_len does not fit 64 bits")
        if n_order is None:
            n_order = len(graph.node_order())
        if exclude is not None:
            exclude = np.ascontiguousarray(np.asarray(exclude) != 0, dtype=np.uint8)
            if exclude.shape != (int(n_order),):
                raise ValueError("exclude needs one entry per node of the order")
        prm = PoContigParams(int(min_contig_len), int(min_nodes), 0)
        edge_contig, edge_pos = np.zeros(len(graph), dtype=np.uint32), np.zeros(len(graph), dtype=np.uint32)
        table = np.zeros(int(n_order) + len(graph), dtype=CONTIG_DTYPE)
        n = ctypes.c_uint64()
        _check(self._h, fn(self._h, graph._ptr, ctypes.byref(prm), _ptr(exclude) if exclude is not None else None, _ptr(edge_contig),
                           _ptr(edge_pos), _ptr(table), ctypes.byref(n)))
        return edge_contig, edge_pos, table[:int(n.value)].copy()

    def contig_stats(self) -> dict:
        return self._stats(self._lib.po_get_contig_stats, PoContigStats)

    def phase_branch(self, bubble, start_of_block, min_spanning_reads: int = 0, threshold: float = 0.0, levels=None,
                     max_candidates: int = 0, cap: Optional[int] = None, want_table: bool = False):
        """``po_phase_branch``: the haplotype extensions of one bubble scored, filtered and -- with ``levels`` -- pruned.
        ``bubble``: a ``phasm_amd.phasing.PackedBubble`` (``pack_bubble``).  ``threshold``: linear, 0 = keep everything;
        ``levels``: None for the kept list as ``branch`` returns it, else the log10 prune levels of
        ``phasing.prune_levels`` (an empty list prunes nothing, as a factor <= 0 does) with ``max_candidates``.  Returns
        ``(cand, ext, rl)`` -- candidate set, extension id (``phasing.ext_digits``) and log10 relative likelihood of every
        entry, in the reference's order -- and with ``want_table`` also S as C * k * P doubles.  ``cap``: write at most this
        many entries (``phase_stats()`` has the full counts); None: all of them."""
        b = bubble
        if not 0 <= int(min_spanning_reads) < 2**32 or not 0 <= int(max_candidates) < 2**32:
            raise ValueError("min_spanning_reads and max_candidates must fit 32 bits")
        lv = np.ascontiguousarray(levels if levels is not None else [], dtype=np.float64)
        arrays = [np.ascontiguousarray(a, dtype=dt) for a, dt in (
            (b.overlap_max, np.int32), (b.aln_off, np.uint32), (b.aln_b, np.uint32), (b.aln_a0, np.int32), (b.aln_a1, np.int32),
            (b.path_off, np.uint32), (b.path_ids, np.uint32), (b.set_off, np.uint32), (b.set_ids, np.uint32), (lv, np.float64))]
        if len(arrays[0]) != b.n_reads or len(arrays[1]) != b.n_reads + 1 or len(arrays[5]) != b.n_paths + 1 or \
                len(arrays[7]) != b.n_cands * b.ploidy + 1:
            raise ValueError("the arrays of the bubble do not have the lengths its sizes give")
        if len({len(arrays[2]), len(arrays[3]), len(arrays[4])}) != 1 or (b.n_reads and len(arrays[2]) != int(arrays[1][-1])) or \
                len(arrays[6]) != int(arrays[5][-1]) or len(arrays[8]) != int(arrays[7][-1]):
            raise ValueError("the arrays of the bubble do not have the lengths its offsets give")
        prm = PoPhaseParams(int(b.ploidy), int(b.n_paths), int(b.n_cands), int(b.n_reads), int(b.n_b), int(bool(start_of_block)),
                            int(min_spanning_reads), int(levels is not None), int(max_candidates), len(lv), float(threshold), 0, 0)
        inp = PoPhaseInput(*[a.ctypes.data if len(a) else None for a in arrays])
        table = np.zeros(b.n_cands * b.ploidy * b.n_paths if want_table else 0, dtype=np.float64)
        room = min(b.n_cands * b.n_paths ** b.ploidy, 1 << 20) if cap is None else int(cap)
        n = ctypes.c_uint64()
        while True:
            cand, ext, rl = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.float64)
            _check(self._h, self._lib.po_phase_branch(self._h, ctypes.byref(prm), ctypes.byref(inp), _ptr(cand), _ptr(ext), _ptr(rl), room,
                                                      _ptr(table), ctypes.byref(n)))
            if cap is not None or n.value <= room:
                break
            room = int(n.value)   # (more than the first guess held: once more, with room for all)
        k = min(room, int(n.value))
        out = (cand[:k].copy(), ext[:k].copy(), rl[:k].copy())
        return out + (table,) if want_table else out

    def phase_stats(self) -> dict:
        return self._stats(self._lib.po_get_phase_stats, PoPhaseStats)

    def phase_walk(self, ploidy: int) -> "DeviceWalk":
        """``po_walk_create``: the candidate sets of a walk along a bubble chain, resident on the device from bubble to bubble
        (``phasm_amd.phasing.phase_chain`` drives it)."""
        return DeviceWalk(self, ploidy)

    def walk_stats(self) -> dict:
        return self._stats(self._lib.po_get_walk_stats, _lib.PoWalkStats)

    def phase_index(self, rows: OverlapResult) -> OverlapResult:
        """``po_phase_index``: the reference's ``read_alignments`` mapping of a row result, on the device.  The result holds
        no rows; it stays valid after ``rows`` is freed and goes to ``phase_relevant``."""
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_phase_index(self._h, rows._ptr, ctypes.byref(r)))
        return OverlapResult(self, r, ALIGNMENT_DTYPE)

    def phase_index_entries(self, index: OverlapResult):
        """``po_phase_index_copy``: ``(offsets, entries)`` -- the entries of read x are ``entries[offsets[x]:offsets[x + 1]]``
        (ALIGNMENT_DTYPE: b, a0, a1, seq), ascending in b."""
        n = ctypes.c_uint64()
        off = np.zeros(len(self) + 1, dtype=np.uint64)
        _check(self._h, self._lib.po_phase_index_copy(index._ptr, _ptr(off), None, 0, ctypes.byref(n)))
        entries = np.zeros(int(n.value), dtype=ALIGNMENT_DTYPE)
        _check(self._h, self._lib.po_phase_index_copy(index._ptr, None, _ptr(entries), len(entries), ctypes.byref(n)))
        return off, entries

    def phase_index_stats(self) -> dict:
        return self._stats(self._lib.po_get_phase_index_stats, PoPhaseIndexStats)

    def phase_relevant(self, index: OverlapResult, cur_graph, prev_graph=(), prev_aligning=(), preds=(), mode: int = 0,
                       min_spanning_reads: int = 0) -> "RelevantReads":
        """``po_phase_relevant``: the relevant reads of one bubble with their alignments and overlap_max, in the arrays
        ``po_phase_branch`` takes.  The lists are oriented read ids (duplicates count once); ``preds``: (read, edge_len) of
        the predecessors of the exit that are plain reads; ``mode`` 0 = spanning, 1 = all."""
        if not 0 <= int(mode) < 2**32 or not 0 <= int(min_spanning_reads) < 2**32:
            raise ValueError("mode and min_spanning_reads must fit 32 bits")
        preds = list(preds)
        lists = [np.ascontiguousarray(a, dtype=np.uint32) for a in (
            list(cur_graph), list(prev_graph), list(prev_aligning), [p[0] for p in preds])]
        plen = np.ascontiguousarray([p[1] for p in preds], dtype=np.int32)
        as_p = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
        prm = PoRelevantParams(int(mode), int(min_spanning_reads), 0, 0)
        inp = PoRelevantInput(as_p(lists[0]), len(lists[0]), as_p(lists[1]), len(lists[1]), as_p(lists[2]), len(lists[2]),
                              as_p(lists[3]), as_p(plen), len(plen))
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_phase_relevant(self._h, index._ptr, ctypes.byref(prm), ctypes.byref(inp), ctypes.byref(r)))
        try:
            d = PoRelevantDims()
            _check(self._h, self._lib.po_relevant_sizes(r, ctypes.byref(d)))
            R, A = int(d.n_relevant), int(d.n_alignments)
            out = RelevantReads(np.zeros(int(d.n_cur_aligning), np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.int32),
                                np.zeros(R + 1, np.uint32), np.zeros(A, np.uint32), np.zeros(A, np.int32), np.zeros(A, np.int32),
                                np.zeros(int(d.n_b), np.uint32), int(d.n_spanning), bool(d.fell_back))
            _check(self._h, self._lib.po_relevant_copy(r, _ptr(out.cur_aligning), _ptr(out.rel_reads), _ptr(out.overlap_max), _ptr(out.aln_off),
                                                       _ptr(out.aln_b), _ptr(out.aln_a0), _ptr(out.aln_a1), _ptr(out.b_reads)))
        finally:
            self._lib.po_result_free(r)
        return out

    def relevant_stats(self) -> dict:
        return self._stats(self._lib.po_get_relevant_stats, PoRelevantStats)

    def spell(self, seq_off, piece_read, piece_take) -> List[bytes]:
        """``po_spell``: the sequences of pieces ``(oriented read, take)`` out of the reads on the device (phasm_amd/spelling.py
        builds the pieces of graph paths).  Sequence s is the concatenation, over the pieces ``seq_off[s]:seq_off[s + 1]``, of
        the first ``take`` bytes of the read, a-z upper-cased.  More than 2^32 - 16 bytes in one call: OverflowError (split
        the call); anything else that is refused: ValueError."""
        seq_off, piece_read, piece_take = spell_arrays(seq_off, piece_read, piece_take)
        inp = PoSpellInput(len(seq_off) - 1, len(piece_read), seq_off.ctypes.data, piece_read.ctypes.data if len(piece_read) else None,
                           piece_take.ctypes.data if len(piece_take) else None)
        r = ctypes.c_void_p()
        st = self._lib.po_spell(self._h, ctypes.byref(inp), ctypes.byref(r))
        if st == _lib.PO_ERR_CAPACITY:
            msg = self._lib.po_last_error(self._h)
            raise OverflowError(msg.decode("utf-8", "replace") if msg else "po_spell: too many bytes in one call")
        _check(self._h, st)
        try:
            n_seqs, n_bytes = ctypes.c_uint64(), ctypes.c_uint64()
            _check(self._h, self._lib.po_spell_sizes(r, ctypes.byref(n_seqs), ctypes.byref(n_bytes)))
            off = np.zeros(int(n_seqs.value) + 1, dtype=np.uint64)
            data = np.zeros(int(n_bytes.value), dtype=np.uint8)
            _check(self._h, self._lib.po_spell_copy(r, _ptr(off), _ptr(data), len(data)))
        finally:
            self._lib.po_result_free(r)
        blob, off = data.tobytes(), off.tolist()
        return [blob[off[s]:off[s + 1]] for s in range(len(off) - 1)]

    def spell_stats(self) -> dict:
        return self._stats(self._lib.po_get_spell_stats, PoSpellStats)

    def phase_paths(self, graph: OverlapResult, max_paths: int = 0) -> "BubblePaths":
        """``po_phase_paths``: for every top-level bubble of a graph result (of the kinds ``layout_bubblechains`` takes, which
        stays valid) its chain and position, the number of simple paths from entrance to exit, the paths themselves where
        they number at most ``max_paths`` (0: counts only), the interior nodes and the predecessors of the exit with their
        edge weights -- a ``phasm_amd.phasing.BubblePaths``.  Too many paths to list in one call: OverflowError (lower
        ``max_paths``)."""
        if not 0 <= int(max_paths) < 2**64:
            raise ValueError("max_paths does not fit 64 bits")
        prm = _lib.PoPathsParams(int(max_paths), 0)
        r = ctypes.c_void_p()
        st = self._lib.po_phase_paths(self._h, graph._ptr, ctypes.byref(prm), ctypes.byref(r))
        if st == _lib.PO_ERR_CAPACITY:
            msg = self._lib.po_last_error(self._h)
            raise OverflowError(msg.decode("utf-8", "replace") if msg else "po_phase_paths: too many paths in one call")
        _check(self._h, st)
        try:
            d = _lib.PoPathsDims()
            _check(self._h, self._lib.po_paths_sizes(r, ctypes.byref(d)))
            nb, npaths = int(d.n_bubbles), int(d.n_listed_paths)
            out = BubblePaths(np.zeros(nb, _lib.BUBBLE_PATHS_DTYPE), np.zeros(nb + 1, np.uint64), np.zeros(int(d.n_inside_nodes), np.uint32),
                              np.zeros(nb + 1, np.uint64), np.zeros(int(d.n_preds), np.uint32), np.zeros(int(d.n_preds), np.int32),
                              np.zeros(nb + 1, np.uint64), np.zeros(npaths + 1, np.uint64), np.zeros(int(d.n_path_nodes), np.uint32))
            _check(self._h, self._lib.po_paths_copy(r, _ptr(out.bubbles), _ptr(out.inside_off), _ptr(out.inside_nodes), _ptr(out.pred_off),
                                                    _ptr(out.pred_node), _ptr(out.pred_weight), _ptr(out.bubble_path_off), _ptr(out.path_off),
                                                    _ptr(out.path_nodes)))
        finally:
            self._lib.po_result_free(r)
        return out

    def paths_stats(self) -> dict:
        return self._stats(self._lib.po_get_paths_stats, _lib.PoPathsStats)

    def phase_paths_resident(self, graph: OverlapResult, max_paths: int = 0) -> "DevicePaths":
        """``po_phase_paths`` with the result KEPT on the device: a ``DevicePaths``, to be closed.  What ``phase_paths`` brings
        home except the listed paths themselves, which are fetched by range or scored where they are
        (``DevicePaths.score_large``).  Too many paths to list in one call: OverflowError (lower ``max_paths``)."""
        if not 0 <= int(max_paths) < 2**64:
            raise ValueError("max_paths does not fit 64 bits")
        prm = _lib.PoPathsParams(int(max_paths), 0)
        r = ctypes.c_void_p()
        st = self._lib.po_phase_paths(self._h, graph._ptr, ctypes.byref(prm), ctypes.byref(r))
        if st == _lib.PO_ERR_CAPACITY:
            msg = self._lib.po_last_error(self._h)
            raise OverflowError(msg.decode("utf-8", "replace") if msg else "po_phase_paths: too many paths in one call")
        _check(self._h, st)
        return DevicePaths(self, r)

    def large_stats(self) -> dict:
        return self._stats(self._lib.po_get_large_stats, _lib.PoLargeStats)

    def graph_from_edges(self, edges, node_order) -> OverlapResult:
        """``po_graph_from_edges``: a graph result from caller-supplied edges (structured EDGE_DTYPE or int array [n, 4]:
        u, v, weight, overlap_len over this handle's oriented reads) and the order of its nodes."""
        edges = np.asarray(edges)
        if edges.dtype != EDGE_DTYPE:
            arr = edges.reshape(-1, 4)
            out = np.empty(len(arr), dtype=EDGE_DTYPE)
            for k, name in enumerate(EDGE_DTYPE.names):
                out[name] = arr[:, k]
            edges = out
        edges = np.ascontiguousarray(edges)
        order = np.ascontiguousarray(np.asarray(node_order, dtype=np.int64).reshape(-1))
        if len(order) and (order.min() < 0 or order.max() >= 2**32):
            raise ValueError("a node of the node order does not fit 32 bits")
        order = order.astype(np.uint32)
        r = ctypes.c_void_p()
        _check(self._h, self._lib.po_graph_from_edges(self._h, _ptr(edges), len(edges), _ptr(order), len(order), ctypes.byref(r)))
        return OverlapResult(self, r, EDGE_DTYPE)

    def node_order_stats(self) -> dict:
        """Times of the two node-order passes of the last ``layout_edges`` call (not part of ``layout_stats``)."""
        return self._stats(self._lib.po_get_node_order_stats, PoNodeOrderStats)

    def tips_stats(self) -> dict:
        return self._stats(self._lib.po_get_tips_stats, PoTipsStats)

    def __len__(self) -> int:
        return int(self._lib.po_num_sequences(self._h))

    def ids(self) -> List[str]:
        out = []
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        for i in range(len(self)):
            self._lib.po_get_id(self._h, i, ctypes.byref(p), ctypes.byref(n))
            out.append(ctypes.string_at(p.value, n.value).decode("utf-8", "surrogateescape") if n.value else "")
        return out

    def lengths(self) -> np.ndarray:
        return np.array([self._lib.po_get_length(self._h, i) for i in range(len(self))], dtype=np.int64)

    def stats(self) -> dict:
        s = PoStats()
        _check(self._h, self._lib.po_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.po_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
