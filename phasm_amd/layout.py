"""Host mirror of stage 1 of ``phasm layout`` -- the consumer of the overlap rows.

The reference (/root/reference/phasm/cli/assembler.py:52-139) reads the GFA2 file twice (segments,
then ``E`` lines), turns every line into a ``LocalAlignment`` (phasm/io/gfa.py:90-104), pushes it
through ``ContainedReads`` / ``MinReadLength`` / ``MinOverlapLength`` / ``MaxOverhang``
(phasm/filter.py:37-122), feeds the survivors to ``build_assembly_graph``
(phasm/assembly_graph.py:136-179) and finally deletes every filtered read in both orientations
(assembler.py:108-126).  Here the same result -- the edge set of the graph at "Final graph"
(assembler.py:136) -- comes from ``po_layout_edges`` on the device, either straight from the rows of
``po_overlaps`` (no file in between) or from a GFA2 file read natively (``po_add_gfa``).

The first two operations of graph cleaning follow on request (``reduce=True`` / ``reduce_assembly_graph``):
``remove_transitive_edges`` (Myers' reduction, phasm/assembly_graph.py:182-264) and ``make_symmetric``
(assembly_graph.py:429-443) as `phasm layout` applies them (assembler.py:145-159), by ``po_layout_reduce`` on
the edges still in HBM, and then the next three (``tips=True`` / ``remove_tips``): ``remove_tips``, ``make_symmetric``
and ``clean_graph`` (assembly_graph.py:267-394, :429-453; assembler.py:161-167) by ``po_layout_tips``, in the reference's
node order.  Cleaning after that point (diamond tips, merging, coverage, bubbles, assembler.py:173 on) is out of scope.
No CPU fallback: without the HIP library and a GPU these functions raise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .overlapper import ExactOverlapper, OverlapResult

# `phasm layout` defaults, assembler.py:469-489
DEFAULTS = dict(min_read_length=0, min_overlap_length=0, max_overhang_abs=1000, max_overhang_rel=0.8)


@dataclass
class AssemblyEdges:
    """Edges of the assembly graph after stage 1: ``edges`` is a structured array (u, v, weight,
    overlap_len) with u, v oriented-read indices into ``ids``; ``contained[i]`` tells that read i (nodes 2i,
    2i+1) was contained in another read and left the graph.  After ``reduce_assembly_graph``: ``edges`` are the
    edges left, ``flags`` has one byte per stage-1 edge in stage-1 order (0 kept, 1 transitive, 2 removed by the
    symmetry pass) and ``reduce_stats`` the counts and times of ``po_layout_reduce``.  After ``remove_tips``: ``edges``
    are the edges left, ``tip_flags`` has one byte per edge that went into tip removal, in that order (0 kept,
    1 incoming-tip edge, 2 outgoing-tip edge, 3 removed by the symmetry pass) and ``tips_stats`` the counts, rounds and
    times of ``po_layout_tips``."""
    edges: np.ndarray
    contained: np.ndarray
    ids: List[str]
    stats: dict
    flags: Optional[np.ndarray] = None
    reduce_stats: Optional[dict] = None
    tip_flags: Optional[np.ndarray] = None
    tips_stats: Optional[dict] = None

    def edge_tuples(self) -> List[Tuple[str, str, int, int]]:
        ids = self.ids
        e = self.edges
        return [(ids[u], ids[v], w, o) for u, v, w, o in
                zip(e["u"].tolist(), e["v"].tolist(), e["weight"].tolist(), e["overlap_len"].tolist())]

    def to_networkx(self):
        """A ``networkx.DiGraph`` with the reference's edge attributes (``weight``, ``overlap_len``)."""
        import networkx
        g = networkx.DiGraph()
        for u, v, w, o in self.edge_tuples():
            g.add_edge(u, v, weight=w, overlap_len=o)
        return g


def reduce_assembly_graph(ov: ExactOverlapper, edges_result: OverlapResult, length_fuzz: int = 1000,
                          contained: Optional[np.ndarray] = None, stats: Optional[dict] = None, tips: bool = False,
                          max_tip_len: int = 4, max_tip_len_bases: int = 5000) -> AssemblyEdges:
    """``remove_transitive_edges(g, length_fuzz)`` + removal + ``make_symmetric`` on a ``layout_edges`` result of
    ``ov`` (which stays valid): the edges left, plus the flag byte of every stage-1 edge.  With ``tips`` the tip
    removal follows on the reduced graph."""
    kept, flags = ov.layout_reduce(edges_result, length_fuzz, want_flags=True)
    try:
        if contained is None:
            contained = np.zeros(len(ov) // 2, dtype=bool)
        stats = stats if stats is not None else ov.layout_stats()
        if tips:
            out = remove_tips(ov, kept, max_tip_len, max_tip_len_bases, contained, stats)
            out.flags, out.reduce_stats = flags, ov.reduce_stats()
            return out
        edges = kept.rows()
    finally:
        kept.free()
    return AssemblyEdges(edges, contained, ov.ids(), stats, flags, ov.reduce_stats())


def remove_tips(ov: ExactOverlapper, edges_result: OverlapResult, max_tip_len: int = 4, max_tip_len_bases: int = 5000,
                contained: Optional[np.ndarray] = None, stats: Optional[dict] = None) -> AssemblyEdges:
    """``remove_tips(g, max_tip_len, max_tip_len_bases)`` + ``make_symmetric`` + ``clean_graph`` on an edge result of
    ``ov`` (which stays valid): the edges left, plus the flag byte of every input edge."""
    kept, tip_flags = ov.layout_tips(edges_result, max_tip_len, max_tip_len_bases, want_flags=True)
    try:
        edges = kept.rows()
    finally:
        kept.free()
    if contained is None:
        contained = np.zeros(len(ov) // 2, dtype=bool)
    return AssemblyEdges(edges, contained, ov.ids(), stats if stats is not None else ov.layout_stats(),
                         tip_flags=tip_flags, tips_stats=ov.tips_stats())


def build_assembly_graph(ov: ExactOverlapper, rows: OverlapResult, min_read_length: int = 0,
                         min_overlap_length: int = 0, max_overhang_abs: int = 1000,
                         max_overhang_rel: float = 0.8, reduce: bool = False, length_fuzz: int = 1000, tips: bool = False,
                         max_tip_len: int = 4, max_tip_len_bases: int = 5000) -> AssemblyEdges:
    """Filters + ``build_assembly_graph`` + contained-read removal on a row result of ``ov``; with ``reduce`` the
    transitive reduction and the symmetry pass as well; with ``tips`` the tip removal (after the reduction when both
    are asked for)."""
    res, removed = ov.layout_edges(rows, min_read_length, min_overlap_length, max_overhang_abs, max_overhang_rel)
    try:
        if reduce:
            return reduce_assembly_graph(ov, res, length_fuzz, removed.astype(bool), ov.layout_stats(), tips, max_tip_len,
                                         max_tip_len_bases)
        if tips:
            return remove_tips(ov, res, max_tip_len, max_tip_len_bases, removed.astype(bool), ov.layout_stats())
        edges = res.rows()
    finally:
        res.free()
    return AssemblyEdges(edges, removed.astype(bool), ov.ids(), ov.layout_stats())


def layout_from_gfa(path: str, device: Optional[int] = None, reduce: bool = False, length_fuzz: int = 1000,
                    tips: bool = False, max_tip_len: int = 4, max_tip_len_bases: int = 5000, **params) -> AssemblyEdges:
    """``phasm layout`` stage 1 from an overlap file: native GFA2 read, then the device passes."""
    ov = ExactOverlapper(device=device)
    try:
        _, rows = ov.add_gfa(path)
        try:
            return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, **{**DEFAULTS, **params})
        finally:
            rows.free()
    finally:
        ov.close()


def load_daligner(ov: ExactOverlapper, db_input, las_input, translations=None) -> OverlapResult:
    """DBdump + LAdump text -> the reads (as segments) and the row result on ``ov``, i.e. the state after
    ``daligner2gfa`` and ``po_add_gfa`` without the file in between (phasm_amd/io/daligner.py ``to_rows``)."""
    from .io import daligner
    names, lengths, rows = daligner.to_rows(db_input, las_input, translations)
    for name, n in zip(names, lengths.tolist()):
        ov.add_segment(name, n)
    return ov.result_from_rows(rows)


def layout_from_daligner(db_input, las_input, translations=None, device: Optional[int] = None, reduce: bool = False,
                         length_fuzz: int = 1000, tips: bool = False, max_tip_len: int = 4, max_tip_len_bases: int = 5000,
                         **params) -> AssemblyEdges:
    """``phasm layout`` stage 1 straight from DAZZ_DB / DALIGNER dump text."""
    ov = ExactOverlapper(device=device)
    try:
        rows = load_daligner(ov, db_input, las_input, translations)
        try:
            return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, **{**DEFAULTS, **params})
        finally:
            rows.free()
    finally:
        ov.close()


def layout_from_overlaps(ov: ExactOverlapper, min_length: int, reduce: bool = False, length_fuzz: int = 1000,
                         tips: bool = False, max_tip_len: int = 4, max_tip_len_bases: int = 5000, **params) -> AssemblyEdges:
    """Overlap + layout stage 1 without the file in between: the rows never leave HBM."""
    rows = ov.overlaps_result(min_length)
    try:
        return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, **{**DEFAULTS, **params})
    finally:
        rows.free()
