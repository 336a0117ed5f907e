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
node order, and ``remove_diamond_tips`` (assembly_graph.py:721-743; assembler.py:173) by ``po_layout_diamonds``
(``remove_diamond_tips`` here).  ``clean_assembly_graph`` / ``clean=True`` runs the whole sequence of assembler.py:145-182
in one call -- reduction, tips, diamond tips, tips again -- and tells for every stage-1 edge which step removed it.
``merge_unambiguous_paths`` / ``merge=True`` adds the last call that changes the graph before `phasm layout` writes it
(assembly_graph.py:456-541; assembler.py:184-186) by ``po_layout_merge``: every non-branching path becomes one ``merged%d``
node, and the result describes the GFA2 file the command writes (``S``, ``F`` and ``E`` lines, phasm/io/gfa.py:281-326).
``average_coverage`` / ``coverage=True`` computes what the command computes next, the average coverage of every edge
(``average_coverage_path``, assembly_graph.py:544-591; assembler.py:190-193), by ``po_layout_coverage`` from all the rows
still in HBM, and ``write_graphml`` writes the graph with that attribute (the counterpart of assembler.py:208-209).
``weakly_connected_components`` is the first step of the command that reads that file, `phasm chain`
(assembler.py:231-310): the components of a graph result by ``po_layout_components``, numbered as networkx yields them;
``chain_components`` runs it on a graph file and ``write_component_graphs`` writes ``component{i}.gfa`` / ``.graphml``.
``strongly_connected_components`` (``po_layout_partition``) and ``superbubble_partitions`` are what superbubble detection
starts with inside each component: ``partition_graph`` (phasm/bubbles.py:32-84).  ``superbubbles``
(``po_layout_superbubbles``) are the superbubbles of the acyclic partitions: ``SuperBubbleFinderDAG`` (bubbles.py:174-381).
``bubble_chains`` (``po_layout_bubblechains``) builds the chains of the bubbles that are not nested:
``build_bubblechains`` (assembly_graph.py:594-652); with them ``write_component_graphs`` also writes
``component{i}.bubblechain{j}.*`` and the node attribute ``bubblechain``.
``identify_contigs`` (``po_layout_contigs``) reports the non-branching paths and single nodes outside the chains:
``identify_contigs`` (assembly_graph.py:655-718); with them ``write_component_graphs`` also writes
``component{i}.contig{j}.*`` and the edge attribute ``contig``: every file `phasm chain` writes.
What follows that point: of `phasm phase` the scoring and pruning of the haplotype extensions at one bubble is
``phasm_amd.phasing`` (``po_phase_branch``), as are the relevant reads of a bubble (``po_phase_index``, ``po_phase_relevant``);
the superbubbles of the cyclic partitions (what the reference reaches through ``graph_to_dag``) come from
``superbubbles(..., cyclic=True)`` (``po_layout_superbubbles_all``, root splitting: DESIGN.md section 3.9t), and with ``cyclic=True`` the chains and the contigs
build on them (``po_layout_bubblechains_all`` / ``po_layout_contigs_all``, ring chains: section 3.9u); the paths still take
the acyclic partitions only.
No CPU fallback: without the HIP library and a GPU these functions raise.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .overlapper import ExactOverlapper, OverlapResult

logger = logging.getLogger("phasm_amd")

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
    times of ``po_layout_tips``.  After ``remove_diamond_tips``: ``diamond_flags`` has one byte per edge that went into
    it (0 kept, 1 in-edge of a removed end node, 2 the in-edge of a removed pred1) and ``diamond_stats`` the counts, rounds
    and times of ``po_layout_diamonds``.  After ``clean_assembly_graph``: ``edges`` are the edges left by the whole
    chain, ``removed_by`` has one byte per stage-1 edge in stage-1 order (``REMOVED_BY``) and ``clean_stats`` the stats of
    the four device calls in order (reduce, tips, diamonds, tips).  After ``merge_unambiguous_paths``: ``edges`` are the
    edges of the merged graph (a node id >= ``len(ids)`` names merged node ``id - len(ids)``), ``merge_flags`` has one
    byte per edge that went into the merge (0 kept as it is, 1 link of a path, 2 kept with a renamed end or a raised
    weight), ``merged_paths`` the tables ``(offsets, members, prefix_lengths, lengths)`` of the merged nodes,
    ``merge_stats`` the counts, rounds and times of ``po_layout_merge``, ``node_order`` the nodes of the merged graph in
    the reference's order and ``node_lengths`` the length of every oriented read.  These five fields are set only by the
    merge (``merge_unambiguous_paths`` or ``merge=True``) and stay ``None`` otherwise.  With ``coverage=True`` (or
    ``coverage_rows``) three more, all in the order of ``edges``: ``coverage_sums`` (structured: ``read_length_sum``,
    ``path_length``), ``avg_coverage`` (float64, the reference's ``avg_coverage`` edge attribute) and ``coverage_stats``
    (``po_get_coverage_stats``); ``None`` unless asked for."""
    edges: np.ndarray
    contained: np.ndarray
    ids: List[str]
    stats: dict
    flags: Optional[np.ndarray] = None
    reduce_stats: Optional[dict] = None
    tip_flags: Optional[np.ndarray] = None
    tips_stats: Optional[dict] = None
    diamond_flags: Optional[np.ndarray] = None
    diamond_stats: Optional[dict] = None
    removed_by: Optional[np.ndarray] = None
    clean_stats: Optional[List[dict]] = None
    merge_flags: Optional[np.ndarray] = None
    merged_paths: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]] = None
    merge_stats: Optional[dict] = None
    node_order: Optional[np.ndarray] = None
    node_lengths: Optional[np.ndarray] = None
    coverage_sums: Optional[np.ndarray] = None
    avg_coverage: Optional[np.ndarray] = None
    coverage_stats: Optional[dict] = None

    def node_name(self, n: int) -> str:
        """The reference's ``str(node)``: the oriented read's id, or ``merged%d+`` for a merged node."""
        n = int(n)
        return self.ids[n] if n < len(self.ids) else "merged%d+" % (n - len(self.ids))

    def node_length(self, n: int) -> int:
        """The reference's ``len(node)`` (needs ``node_lengths``, which ``merge_unambiguous_paths`` fills in)."""
        n = int(n)
        if n < len(self.ids):
            if self.node_lengths is None:
                raise ValueError("this AssemblyEdges carries no read lengths")
            return int(self.node_lengths[n])
        if self.merged_paths is None or n - len(self.ids) >= len(self.merged_paths[3]):
            raise ValueError("node %d is no node of this graph" % n)
        return int(self.merged_paths[3][n - len(self.ids)])

    def edge_tuples(self) -> List[Tuple[str, str, int, int]]:
        ids = self.ids
        e = self.edges
        if self.merged_paths is not None:
            ids = [self.node_name(n) for n in range(len(ids) + len(self.merged_paths[3]))]
        return [(ids[u], ids[v], w, o) for u, v, w, o in
                zip(e["u"].tolist(), e["v"].tolist(), e["weight"].tolist(), e["overlap_len"].tolist())]

    def to_networkx(self):
        """A ``networkx.DiGraph`` with the reference's edge attributes (``weight``, ``overlap_len`` and, when the
        coverage was asked for, ``avg_coverage``)."""
        import networkx
        g = networkx.DiGraph()
        for u, v, w, o in self.edge_tuples():
            g.add_edge(u, v, weight=w, overlap_len=o)
        if self.avg_coverage is not None:
            for (u, v, _, _), c in zip(self.edge_tuples(), self.avg_coverage.tolist()):
                g[u][v]["avg_coverage"] = c
        return g


def _quotients(sums: np.ndarray) -> np.ndarray:
    """``read_length_sum / path_length`` per edge as the reference computes it: both are exact integers below 2**53, so
    the IEEE double quotient is Python's ``int / int`` bit for bit.  A zero path length raises like the reference."""
    if len(sums) and (sums["path_length"] == 0).any():
        raise ZeroDivisionError("division by zero: an edge with path_length == 0")
    return sums["read_length_sum"].astype(np.float64) / sums["path_length"].astype(np.float64)


def _coverage_into(out: "AssemblyEdges", ov: ExactOverlapper, graph_res: OverlapResult,
                   rows_res: Optional[OverlapResult]) -> "AssemblyEdges":
    """Fills the three coverage fields of ``out`` for the graph ``graph_res`` (whose edges ``out.edges`` are) when rows are given."""
    if rows_res is not None:
        out.coverage_sums, out.coverage_stats = ov.layout_coverage(graph_res, rows_res), ov.coverage_stats()
        out.avg_coverage = _quotients(out.coverage_sums)
    return out


def average_coverage(ov: ExactOverlapper, graph_res: OverlapResult, rows_res: OverlapResult) -> np.ndarray:
    """The reference's ``average_coverage_path(g, read_alignments, [u, v])`` for every edge of ``graph_res`` (an edge result
    or a merged graph of ``ov``), ``read_alignments`` being every row of ``rows_res``: float64, in the graph's edge order."""
    return _quotients(ov.layout_coverage(graph_res, rows_res))


def write_graphml(f, g: "AssemblyEdges", bubblechain: Optional[dict] = None, contig: Optional[dict] = None) -> int:
    """The graph ``g`` as GraphML with the reference's attribute names: nodes named by ``node_name`` (the nodes of
    ``node_order`` where the result carries one, else the ends of the edges in order of appearance), edge data ``weight``,
    ``overlap_len`` and, when present, ``avg_coverage`` (written with ``repr``: it reads back to the same double).  With
    ``bubblechain`` ({node name: number}, None: no such attribute) the nodes it names carry the node attribute
    ``bubblechain`` (long), as `phasm chain` marks them (assembler.py:277-278); with ``contig`` ({index of the edge in
    ``g.edge_tuples()``: number}, None: no such attribute) the edges it names carry the edge attribute ``contig`` (long,
    assembler.py:293-295).  Returns the number of edges."""
    from xml.sax.saxutils import escape, quoteattr
    names = g.edge_tuples()
    nodes = [g.node_name(n) for n in g.node_order.tolist()] if g.node_order is not None else []
    seen = set(nodes)
    for u, v, _, _ in names:
        for n in (u, v):
            if n not in seen:
                seen.add(n)
                nodes.append(n)
    cov = g.avg_coverage.tolist() if g.avg_coverage is not None else None
    f.write('<?xml version="1.0" encoding="utf-8"?>\n<graphml xmlns="http://graphml.graphdrawing.org/xmlns" '
            'xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" xsi:schemaLocation="http://graphml.graphdrawing.org/xmlns '
            'http://graphml.graphdrawing.org/xmlns/1.0/graphml.xsd">\n')
    f.write('  <key id="d0" for="edge" attr.name="weight" attr.type="long" />\n'
            '  <key id="d1" for="edge" attr.name="overlap_len" attr.type="long" />\n')
    if cov is not None:
        f.write('  <key id="d2" for="edge" attr.name="avg_coverage" attr.type="double" />\n')
    if bubblechain is not None:
        f.write('  <key id="d3" for="node" attr.name="bubblechain" attr.type="long" />\n')
    if contig is not None:
        f.write('  <key id="d4" for="edge" attr.name="contig" attr.type="long" />\n')
    f.write('  <graph edgedefault="directed">\n')
    if bubblechain is None:
        f.write("".join("    <node id=%s />\n" % quoteattr(n) for n in nodes))
    else:
        f.write("".join('    <node id=%s>\n      <data key="d3">%d</data>\n    </node>\n' % (quoteattr(n), bubblechain[n])
                        if n in bubblechain else "    <node id=%s />\n" % quoteattr(n) for n in nodes))
    for i, (u, v, w, o) in enumerate(names):
        f.write('    <edge source=%s target=%s>\n      <data key="d0">%d</data>\n      <data key="d1">%d</data>\n'
                % (quoteattr(u), quoteattr(v), w, o))
        if cov is not None:
            f.write('      <data key="d2">%s</data>\n' % escape(repr(cov[i])))
        if contig is not None and i in contig:
            f.write('      <data key="d4">%d</data>\n' % contig[i])
        f.write("    </edge>\n")
    f.write("  </graph>\n</graphml>\n")
    return len(names)


def reduce_assembly_graph(ov: ExactOverlapper, edges_result: OverlapResult, length_fuzz: int = 1000,
                          contained: Optional[np.ndarray] = None, stats: Optional[dict] = None, tips: bool = False,
                          max_tip_len: int = 4, max_tip_len_bases: int = 5000,
                          coverage_rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    """``remove_transitive_edges(g, length_fuzz)`` + removal + ``make_symmetric`` on a ``layout_edges`` result of
    ``ov`` (which stays valid): the edges left, plus the flag byte of every stage-1 edge.  With ``tips`` the tip
    removal follows on the reduced graph.  With ``coverage_rows`` (here and in the functions below: the row result the
    graph came from) the coverage of every edge left is computed as well."""
    kept, flags = ov.layout_reduce(edges_result, length_fuzz, want_flags=True)
    try:
        if contained is None:
            contained = np.zeros(len(ov) // 2, dtype=bool)
        stats = stats if stats is not None else ov.layout_stats()
        if tips:
            rstats = ov.reduce_stats()
            out = remove_tips(ov, kept, max_tip_len, max_tip_len_bases, contained, stats, coverage_rows)
            out.flags, out.reduce_stats = flags, rstats
            return out
        out = AssemblyEdges(kept.rows(), contained, ov.ids(), stats, flags, ov.reduce_stats())
        return _coverage_into(out, ov, kept, coverage_rows)
    finally:
        kept.free()


def remove_tips(ov: ExactOverlapper, edges_result: OverlapResult, max_tip_len: int = 4, max_tip_len_bases: int = 5000,
                contained: Optional[np.ndarray] = None, stats: Optional[dict] = None,
                coverage_rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    """``remove_tips(g, max_tip_len, max_tip_len_bases)`` + ``make_symmetric`` + ``clean_graph`` on an edge result of
    ``ov`` (which stays valid): the edges left, plus the flag byte of every input edge."""
    kept, tip_flags = ov.layout_tips(edges_result, max_tip_len, max_tip_len_bases, want_flags=True)
    try:
        if contained is None:
            contained = np.zeros(len(ov) // 2, dtype=bool)
        out = AssemblyEdges(kept.rows(), contained, ov.ids(), stats if stats is not None else ov.layout_stats(),
                            tip_flags=tip_flags, tips_stats=ov.tips_stats())
        return _coverage_into(out, ov, kept, coverage_rows)
    finally:
        kept.free()


def remove_diamond_tips(ov: ExactOverlapper, edges_result: OverlapResult, contained: Optional[np.ndarray] = None,
                        stats: Optional[dict] = None, coverage_rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    """``remove_diamond_tips(g)`` on an edge result of ``ov`` (which stays valid): the edges left, plus the flag byte of
    every input edge.  Nodes the call leaves without an edge stay nodes (no ``clean_graph`` follows in the reference)."""
    kept, diamond_flags = ov.layout_diamonds(edges_result, want_flags=True)
    try:
        if contained is None:
            contained = np.zeros(len(ov) // 2, dtype=bool)
        out = AssemblyEdges(kept.rows(), contained, ov.ids(), stats if stats is not None else ov.layout_stats(),
                            diamond_flags=diamond_flags, diamond_stats=ov.diamond_stats())
        return _coverage_into(out, ov, kept, coverage_rows)
    finally:
        kept.free()


def _merge_into(out: AssemblyEdges, ov: ExactOverlapper, edges_result: OverlapResult,
                coverage_rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    merged, flags = ov.layout_merge(edges_result, want_flags=True)
    try:
        out.edges, out.merge_flags, out.merge_stats = merged.rows(), flags, ov.merge_stats()
        out.merged_paths, out.node_order, out.node_lengths = merged.merged_paths(), merged.node_order(), ov.lengths()
        _coverage_into(out, ov, merged, coverage_rows)
    finally:
        merged.free()
    return out


def merge_unambiguous_paths(ov: ExactOverlapper, edges_result: OverlapResult, contained: Optional[np.ndarray] = None,
                            stats: Optional[dict] = None, coverage_rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    """``merge_unambiguous_paths(g)`` on an edge result of ``ov`` (which stays valid): the merged graph's edges, the flag
    byte of every input edge, the tables of the merged nodes and the node order."""
    if contained is None:
        contained = np.zeros(len(ov) // 2, dtype=bool)
    out = AssemblyEdges(np.empty(0), contained, ov.ids(), stats if stats is not None else ov.layout_stats())
    return _merge_into(out, ov, edges_result, coverage_rows)


def write_merged_graph(f, g: AssemblyEdges) -> int:
    """What the reference's ``gfa2_write_graph`` (phasm/io/gfa.py:281-326) writes for the merged graph ``g`` (a result of
    ``merge_unambiguous_paths`` or of ``merge=True``): the header; for every node in node order one ``S`` line per segment
    name at its first occurrence, followed for a merged node by its ``F`` lines; then the ``E`` lines, in the result's own
    order (the reference's adjacency order is not reproduced).  Returns the number of ``E`` lines."""
    from .io import gfa
    if g.merged_paths is None or g.node_order is None:
        raise ValueError("write_merged_graph needs the result of merge_unambiguous_paths")
    offsets, members, prefix, lengths = g.merged_paths
    n_ids = len(g.ids)
    f.write(gfa.gfa_header())
    segments = set()
    for n in g.node_order.tolist():
        name = g.node_name(n)[:-1]
        if name in segments:
            continue
        segments.add(name)
        f.write(gfa.gfa_line("S", name, g.node_length(n), "*"))
        if n >= n_ids:
            k = n - n_ids
            lo, hi = int(offsets[k]), int(offsets[k + 1])
            total, cur, length = int(prefix[lo:hi].sum()), 0, int(lengths[k])
            # The reference takes a falsy prefix for the last read (gfa.py:301-307).  Stage 1 never emits a weight <= 0,
            # so the prefix of every read but a path's last is positive and the two tests agree.
            for read, p in zip(members[lo:hi].tolist(), prefix[lo:hi].tolist()):
                f.write(gfa.gfa_line("F", name, g.ids[read], cur, cur + p if p else length, 0, p if p else length - total, "*"))
                cur += p
    e = g.edges
    node_len = np.concatenate([np.asarray(g.node_lengths, dtype=np.int64), np.asarray(lengths, dtype=np.int64)])
    names = [g.node_name(n) for n in range(n_ids + len(lengths))]
    f.write("".join("E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % t for t in
                    zip([names[u] for u in e["u"].tolist()], [names[v] for v in e["v"].tolist()], e["weight"].tolist(),
                        node_len[e["u"]].tolist() if len(e) else [], e["overlap_len"].tolist())))
    return len(e)


# ``AssemblyEdges.removed_by``: which step of assembler.py:145-182 removed a stage-1 edge
REMOVED_BY = {0: "kept", 1: "transitive", 2: "asymmetric after the reduction", 3: "incoming tip", 4: "outgoing tip",
              5: "asymmetric after the tips", 6: "in-edge of a diamond's end node", 7: "in-edge of a diamond's pred1",
              8: "incoming tip (stage 2)", 9: "outgoing tip (stage 2)", 10: "asymmetric after the tips (stage 2)"}
_REMOVED_BY_BASE = (0, 2, 5, 7)   # reduce flags 1-2, tips 1-3, diamonds 1-2, tips 1-3


def clean_assembly_graph(ov: ExactOverlapper, edges_result: OverlapResult, length_fuzz: int = 1000, max_tip_len: int = 4,
                         max_tip_len_bases: int = 5000, contained: Optional[np.ndarray] = None,
                         stats: Optional[dict] = None, merge: bool = False, coverage: bool = False,
                         rows: Optional[OverlapResult] = None) -> AssemblyEdges:
    """Graph cleaning as `phasm layout` runs it up to the merging of paths (assembler.py:145-182) on a ``layout_edges``
    result of ``ov`` (which stays valid): reduction + symmetry, tips with both bounds + symmetry + isolated nodes, diamond
    tips, tips again with ``max_tip_len`` and the function's own default of 5000 bases (the reference's second call
    passes no base bound) + symmetry + isolated nodes.  Four device calls; the edges stay in HBM in between.  With
    ``merge`` the merging of unambiguous paths follows as a fifth (assembler.py:184-186): ``removed_by`` stays what the
    cleaning made it -- a link of a path is not removed by cleaning -- and ``merge_flags`` refers to the edges that went
    into the merge, those with ``removed_by == 0`` in stage-1 order.  With ``coverage`` the average coverage of every
    edge of the graph the call ends with follows (assembler.py:190-193); it needs ``rows``, the row result the stage-1
    graph was built from."""
    if coverage and rows is None:
        raise ValueError("coverage=True needs the row result the graph was built from (rows=...)")
    coverage_rows = rows if coverage else None
    steps = (lambda r: ov.layout_reduce(r, length_fuzz, want_flags=True), ov.reduce_stats), \
            (lambda r: ov.layout_tips(r, max_tip_len, max_tip_len_bases, want_flags=True), ov.tips_stats), \
            (lambda r: ov.layout_diamonds(r, want_flags=True), ov.diamond_stats), \
            (lambda r: ov.layout_tips(r, max_tip_len, 5000, want_flags=True), ov.tips_stats)
    removed_by = np.zeros(len(edges_result), dtype=np.uint8)
    live = np.arange(len(edges_result))
    clean_stats = []
    cur = edges_result
    try:
        for (call, call_stats), base in zip(steps, _REMOVED_BY_BASE):
            kept, flags = call(cur)
            if cur is not edges_result:
                cur.free()
            cur = kept
            clean_stats.append(call_stats())
            removed_by[live[flags != 0]] = flags[flags != 0] + base
            live = live[flags == 0]
        if contained is None:
            contained = np.zeros(len(ov) // 2, dtype=bool)
        out = AssemblyEdges(np.empty(0), contained, ov.ids(), stats if stats is not None else ov.layout_stats(),
                            removed_by=removed_by, clean_stats=clean_stats)
        if merge:
            _merge_into(out, ov, cur, coverage_rows)
        else:
            out.edges = cur.rows()
            _coverage_into(out, ov, cur, coverage_rows)
    finally:
        if cur is not edges_result:
            cur.free()
    return out


def build_assembly_graph(ov: ExactOverlapper, rows: OverlapResult, min_read_length: int = 0,
                         min_overlap_length: int = 0, max_overhang_abs: int = 1000,
                         max_overhang_rel: float = 0.8, reduce: bool = False, length_fuzz: int = 1000, tips: bool = False,
                         max_tip_len: int = 4, max_tip_len_bases: int = 5000, clean: bool = False,
                         merge: bool = False, coverage: bool = False) -> AssemblyEdges:
    """Filters + ``build_assembly_graph`` + contained-read removal on a row result of ``ov``; with ``reduce`` the
    transitive reduction and the symmetry pass as well; with ``tips`` the tip removal (after the reduction when both
    are asked for); with ``clean`` the whole of ``clean_assembly_graph`` instead of either; with ``merge`` (which implies
    ``clean``) the merging of unambiguous paths after it; with ``coverage`` the average coverage of every edge of the
    graph the call ends with."""
    res, removed = ov.layout_edges(rows, min_read_length, min_overlap_length, max_overhang_abs, max_overhang_rel)
    coverage_rows = rows if coverage else None
    try:
        if clean or merge:
            return clean_assembly_graph(ov, res, length_fuzz, max_tip_len, max_tip_len_bases, removed.astype(bool), ov.layout_stats(),
                                        merge=merge, coverage=coverage, rows=coverage_rows)
        if reduce:
            return reduce_assembly_graph(ov, res, length_fuzz, removed.astype(bool), ov.layout_stats(), tips, max_tip_len,
                                         max_tip_len_bases, coverage_rows)
        if tips:
            return remove_tips(ov, res, max_tip_len, max_tip_len_bases, removed.astype(bool), ov.layout_stats(), coverage_rows)
        out = AssemblyEdges(res.rows(), removed.astype(bool), ov.ids(), ov.layout_stats())
        return _coverage_into(out, ov, res, coverage_rows)
    finally:
        res.free()


def layout_from_gfa(path: str, device: Optional[int] = None, reduce: bool = False, length_fuzz: int = 1000,
                    tips: bool = False, max_tip_len: int = 4, max_tip_len_bases: int = 5000, clean: bool = False,
                    merge: bool = False, coverage: bool = False, **params) -> AssemblyEdges:
    """``phasm layout`` stage 1 from an overlap file: native GFA2 read, then the device passes."""
    ov = ExactOverlapper(device=device)
    try:
        _, rows = ov.add_gfa(path)
        try:
            return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, clean=clean, merge=merge, coverage=coverage, **{**DEFAULTS, **params})
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
                         clean: bool = False, merge: bool = False, coverage: bool = False, **params) -> AssemblyEdges:
    """``phasm layout`` stage 1 straight from DAZZ_DB / DALIGNER dump text."""
    ov = ExactOverlapper(device=device)
    try:
        rows = load_daligner(ov, db_input, las_input, translations)
        try:
            return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, clean=clean, merge=merge, coverage=coverage, **{**DEFAULTS, **params})
        finally:
            rows.free()
    finally:
        ov.close()


def layout_from_overlaps(ov: ExactOverlapper, min_length: int, reduce: bool = False, length_fuzz: int = 1000,
                         tips: bool = False, max_tip_len: int = 4, max_tip_len_bases: int = 5000, clean: bool = False,
                         merge: bool = False, coverage: bool = False, **params) -> AssemblyEdges:
    """Overlap + layout stage 1 without the file in between: the rows never leave HBM."""
    rows = ov.overlaps_result(min_length)
    try:
        return build_assembly_graph(ov, rows, reduce=reduce, length_fuzz=length_fuzz, tips=tips, max_tip_len=max_tip_len,
                                        max_tip_len_bases=max_tip_len_bases, clean=clean, merge=merge, coverage=coverage, **{**DEFAULTS, **params})
    finally:
        rows.free()


# ---- the first step of `phasm chain`: weakly connected components (assembler.py:231-310) --------------------------------

@dataclass
class Components:
    """The weakly connected components of a graph result.  ``node_order``: the graph's nodes in the reference's order;
    ``component_of_node``: parallel to it; ``component_of_edge``: the component of u of every edge, in the graph's edge
    order; ``table``: structured (``first_node``, ``n_nodes``, ``n_edges``), one entry per component -- component i is the
    i-th in the order of each component's lowest-ranked node, what ``networkx.weakly_connected_components`` yields;
    ``stats``: ``po_get_components_stats``."""
    node_order: np.ndarray
    component_of_node: np.ndarray
    component_of_edge: np.ndarray
    table: np.ndarray
    stats: dict

    def __len__(self) -> int:
        return len(self.table)

    def edges_of(self, i: int) -> np.ndarray:
        """The indices of the edges of component ``i``, in the graph's edge order."""
        # (grouping is done here, not on the device: it needs a stable sort, and the writers touch every edge anyway)
        if not hasattr(self, "_edge_group"):
            self._edge_group = _groups(self.component_of_edge, len(self), np.arange(len(self.component_of_edge)))
        by, off = self._edge_group
        return by[off[i]:off[i + 1]]

    def nodes_of(self, i: int) -> np.ndarray:
        """The nodes of component ``i``, in node order."""
        if not hasattr(self, "_node_group"):
            self._node_group = _groups(self.component_of_node, len(self), np.arange(len(self.component_of_node)))
        by, off = self._node_group
        return self.node_order[by[off[i]:off[i + 1]]]


def weakly_connected_components(ov: ExactOverlapper, graph_res: OverlapResult) -> Components:
    """``networkx.weakly_connected_components`` on a graph result of ``ov`` (an edge result, a merged graph or a
    ``graph_from_edges`` result), which stays valid and in HBM; the numbering follows the result's own node order."""
    order = graph_res.node_order()
    nodes, edges, table = ov.layout_components(graph_res, len(order))
    return Components(order, nodes, edges, table, ov.components_stats())


# ---- the partition superbubble detection starts with (partition_graph, phasm/bubbles.py:32-84) ---------------------------

@dataclass
class StrongComponents:
    """The strongly connected components of a graph result and what ``partition_graph`` makes of them
    (``po_layout_partition``).  ``node_order``: the graph's nodes in the reference's order; ``scc_of_node`` and
    ``node_flags`` (``_lib.PART_*`` bits): parallel to it; ``edge_class``: the class byte of every edge and ``scc_of_edge``
    the SCC of its u, in the graph's edge order; ``table``: structured (``first_node``, ``n_nodes``, ``n_edges``,
    ``n_r_in``, ``n_re_out``), one entry per SCC -- SCC i is the i-th in the order of each SCC's lowest-ranked node (not
    the DFS order in which networkx yields them); ``stats``: ``po_get_partition_stats``."""
    node_order: np.ndarray
    scc_of_node: np.ndarray
    node_flags: np.ndarray
    edge_class: np.ndarray
    scc_of_edge: np.ndarray
    table: np.ndarray
    stats: dict

    def __len__(self) -> int:
        return len(self.table)


def strongly_connected_components(ov: ExactOverlapper, graph_res: OverlapResult) -> StrongComponents:
    """``po_layout_partition`` on a graph result of ``ov`` (an edge result, a merged graph or a ``graph_from_edges``
    result), which stays valid and in HBM; the numbering follows the result's own node order."""
    order = graph_res.node_order()
    nodes, flags, classes, table = ov.layout_partition(graph_res, len(order))
    stats = ov.partition_stats()
    if len(graph_res):
        u = graph_res.rows()["u"].astype(np.int64)
        rank = np.zeros(int(max(order.max(), u.max())) + 1, dtype=np.int64)
        rank[order] = np.arange(len(order))
        scc_of_edge = nodes[rank[u]]
    else:
        scc_of_edge = np.zeros(0, dtype=np.uint32)
    return StrongComponents(order, nodes, flags, classes, scc_of_edge, table, stats)


@dataclass
class Partition:
    """One subgraph ``partition_graph(component)`` yields.  ``nodes``: its members, in node order; ``edges``: the indices
    of its real edges, in the graph's edge order; ``r_targets`` / ``re_sources``: the nodes v / u of the artificial edges
    ``('r_', v)`` / ``(u, 're_')``, in node order; ``scc``: the SCC of a cyclic partition, None for the acyclic one;
    ``number_of_nodes`` / ``number_of_edges``: of the reference's subgraph, artificial nodes and edges included;
    ``num_sources`` / ``num_sinks``: what ``find_superbubbles`` counts and logs (phasm/bubbles.py:403-406)."""
    component: int
    scc: Optional[int]
    acyclic: bool
    nodes: np.ndarray
    edges: np.ndarray
    r_targets: np.ndarray
    re_sources: np.ndarray
    number_of_nodes: int
    number_of_edges: int
    num_sources: int
    num_sinks: int


def _groups(of: np.ndarray, n_groups: int, among: np.ndarray):
    """(indices of ``among`` sorted by their group, stably; the start of every group in them)."""
    key = of[among].astype(np.int64)
    by = among[np.argsort(key, kind="stable")]
    return by, np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_groups))]).astype(np.int64)


def superbubble_partitions(sccs: StrongComponents, components: Components) -> List[List[Partition]]:
    """Per weakly connected component, the partitions ``partition_graph`` yields on it: its non-singleton SCCs in SCC
    order (``acyclic`` False), then exactly one acyclic partition of its singletons, even when that is empty.  The
    grouping is done with numpy on the host, like ``Components.edges_of``."""
    from ._lib import PART_R_IN, PART_RE_OUT, PART_START, PART_SINK
    order, n_comp, n_scc = sccs.node_order, len(components), len(sccs)
    flags = sccs.node_flags
    single_scc = sccs.table["n_nodes"] == 1
    single_node = single_scc[sccs.scc_of_node] if len(order) else np.zeros(0, dtype=bool)
    comp_of_scc = np.zeros(n_scc, dtype=np.int64)
    comp_of_scc[sccs.scc_of_node] = components.component_of_node
    ranks, eids = np.arange(len(order)), np.arange(len(sccs.edge_class))
    cyc_nodes, cyc_noff = _groups(sccs.scc_of_node, n_scc, ranks[~single_node])
    cyc_edges, cyc_eoff = _groups(sccs.scc_of_edge, n_scc, eids[sccs.edge_class == 0])
    acy_nodes, acy_noff = _groups(components.component_of_node, n_comp, ranks[single_node])
    acy_edges, acy_eoff = _groups(components.component_of_edge, n_comp, eids[sccs.edge_class == 1])
    sccs_by_comp, scc_off = _groups(comp_of_scc, n_comp, np.flatnonzero(~single_scc))

    def make(comp, scc, r, e, in_bits, out_bits):
        r_t, re_s = order[r[(flags[r] & in_bits) != 0]], order[r[(flags[r] & out_bits) != 0]]
        return Partition(comp, scc, scc is None, order[r], e, r_t, re_s, len(r) + (len(r_t) > 0) + (len(re_s) > 0),
                         len(e) + len(r_t) + len(re_s), int(len(r_t) > 0), int(len(re_s) > 0))

    out = []
    for c in range(n_comp):
        parts = []
        for k in sccs_by_comp[scc_off[c]:scc_off[c + 1]].tolist():
            parts.append(make(c, k, cyc_nodes[cyc_noff[k]:cyc_noff[k + 1]], cyc_edges[cyc_eoff[k]:cyc_eoff[k + 1]], PART_R_IN, PART_RE_OUT))
        parts.append(make(c, None, acy_nodes[acy_noff[c]:acy_noff[c + 1]], acy_edges[acy_eoff[c]:acy_eoff[c + 1]],
                          PART_R_IN | PART_START, PART_RE_OUT | PART_SINK))
        out.append(parts)
    return out


# ---- the superbubbles of the acyclic partitions (SuperBubbleFinderDAG, phasm/bubbles.py:174-381) ------------------------------

@dataclass
class Superbubbles:
    """The superbubbles of the acyclic partitions of a graph result (``po_layout_superbubbles``).  ``node_order``: the
    graph's nodes in the reference's order; ``node_exit`` / ``node_inside`` (node ids, ``_lib.NO_NODE`` where there is
    none) and ``node_flags`` (``_lib.SB_*`` bits): parallel to it; ``table``: structured (``entrance``, ``exit``,
    ``n_inside``, ``nested``), one entry per superbubble in the order of the entrances' ranks (the reference's finder yields
    them in another order); ``stats``: ``po_get_superbubble_stats``."""
    node_order: np.ndarray
    node_exit: np.ndarray
    node_inside: np.ndarray
    node_flags: np.ndarray
    table: np.ndarray
    stats: dict

    def __len__(self) -> int:
        return len(self.table)

    def pairs(self, nested: bool = True) -> List[tuple]:
        """The (entrance, exit) pairs: what ``SuperBubbleFinderDAG(partition, report_nested=nested)`` reports, in table order."""
        t = self.table if nested else self.table[self.table["nested"] == 0]
        return list(zip(t["entrance"].tolist(), t["exit"].tolist()))

    def nodes(self, entrance: int) -> np.ndarray:
        """``superbubble_nodes(g, entrance, exit)`` in node order: the two ends and every node whose chain of
        ``node_inside`` reaches the entrance."""
        from ._lib import NO_NODE, SB_ENTRANCE
        if not hasattr(self, "_held"):
            held = self.node_inside != NO_NODE
            self._held = _groups_by_value(self.node_inside[held], np.flatnonzero(held))
            self._rank = {int(n): r for r, n in enumerate(self.node_order.tolist())}
        r = self._rank.get(int(entrance))
        if r is None or not self.node_flags[r] & SB_ENTRANCE:
            raise KeyError("node %d enters no superbubble" % entrance)
        members, work = [r, self._rank[int(self.node_exit[r])]], [int(entrance)]
        while work:   # (every node is held by one bubble: each is visited once)
            for x in self._held.get(work.pop(), ()):
                members.append(x)
                if self.node_flags[x] & SB_ENTRANCE:
                    work.append(int(self.node_order[x]))
        return self.node_order[np.unique(np.asarray(members, dtype=np.int64))]


def _groups_by_value(values: np.ndarray, ranks: np.ndarray) -> dict:
    """{value: the ranks that carry it, ascending}."""
    out = {}
    for v, r in zip(values.tolist(), ranks.tolist()):
        out.setdefault(v, []).append(r)
    return out


def superbubbles(ov, graph_res: Optional[OverlapResult], cyclic: bool = False) -> Superbubbles:
    """``po_layout_superbubbles`` on a graph result of ``ov`` (an edge result, a merged graph or a ``graph_from_edges``
    result), which stays valid and in HBM.  ``cyclic=True``: ``po_layout_superbubbles_all`` instead -- the superbubbles of
    the whole graph, those of the cyclic partitions included; ``ov`` may then be a
    ``cyclic.HostSuperbubblesAll``, which holds its own graph (``graph_res`` is ignored)."""
    if cyclic:
        order = graph_res.node_order() if isinstance(ov, ExactOverlapper) else ov.node_order()
        node_exit, node_inside, flags, table = ov.layout_superbubbles_all(graph_res, len(order))
        return Superbubbles(order, node_exit, node_inside, flags, table, ov.superbubble_all_stats())
    order = graph_res.node_order()
    node_exit, node_inside, flags, table = ov.layout_superbubbles(graph_res, len(order))
    return Superbubbles(order, node_exit, node_inside, flags, table, ov.superbubble_stats())


_superbubbles = superbubbles   # (chain_components has an argument of that name)


# ---- the bubble chains (build_bubblechains, phasm/assembly_graph.py:594-652) -------------------------------------------------

@dataclass
class BubbleChains:
    """The bubble chains of a graph result (``po_layout_bubblechains``).  ``node_order``: the graph's nodes in the
    reference's order; ``node_chain`` / ``node_bubble`` (``_lib.NO_NODE`` where there is none): parallel to it, the chain of
    the node and the position in that chain of the top-level bubble that holds it; ``edge_chain``: the chain that holds both
    ends of every edge, in the graph's edge order; ``table``: structured (``first_entrance``, ``last_exit``, ``n_bubbles``,
    ``n_nodes``, ``n_edges``), one entry per chain in the order of the heads' ranks (the reference numbers them in the
    iteration order of a Python set); ``node_exit``: ``Superbubbles.node_exit`` of the same graph; ``stats``:
    ``po_get_bubblechain_stats``."""
    node_order: np.ndarray
    node_chain: np.ndarray
    node_bubble: np.ndarray
    edge_chain: np.ndarray
    table: np.ndarray
    node_exit: np.ndarray
    stats: dict

    def __len__(self) -> int:
        return len(self.table)

    def _among(self, of: np.ndarray):
        from ._lib import NO_NODE
        return _groups(of, len(self), np.flatnonzero(of != NO_NODE))

    def nodes_of(self, j: int) -> np.ndarray:
        """The nodes of chain ``j``, in node order: what ``build_bubblechains`` yields as a subgraph."""
        if not hasattr(self, "_node_group"):
            self._node_group = self._among(self.node_chain)
        by, off = self._node_group
        return self.node_order[by[off[j]:off[j + 1]]]

    def edges_of(self, j: int) -> np.ndarray:
        """The indices of the edges of chain ``j``, in the graph's edge order."""
        if not hasattr(self, "_edge_group"):
            self._edge_group = self._among(self.edge_chain)
        by, off = self._edge_group
        return by[off[j]:off[j + 1]]

    def bubbles_of(self, j: int) -> List[tuple]:
        """The (entrance, exit) pairs of the top-level bubbles of chain ``j``, in chain order."""
        if not hasattr(self, "_rank"):
            self._rank = {int(n): r for r, n in enumerate(self.node_order.tolist())}
        out, s = [], int(self.table["first_entrance"][j])
        for _ in range(int(self.table["n_bubbles"][j])):
            t = int(self.node_exit[self._rank[s]])
            out.append((s, t))
            s = t
        return out


def bubble_chains(ov, graph_res: Optional[OverlapResult], min_nodes: int = 1, superbubbles: Optional[Superbubbles] = None,
                  cyclic: bool = False) -> BubbleChains:
    """``po_layout_bubblechains`` on a graph result of ``ov`` (an edge result, a merged graph or a ``graph_from_edges``
    result), which stays valid and in HBM; ``superbubbles``: ``layout.superbubbles`` of the same graph, if the caller has
    them (computed here otherwise: ``bubbles_of`` reads the exits from them).  ``cyclic=True``:
    ``po_layout_bubblechains_all`` instead -- the chains behind the superbubbles of the whole graph, RING CHAINS included
    (DESIGN.md section 3.9u); ``superbubbles`` are then those of ``superbubbles(..., cyclic=True)``, so ``bubbles_of`` walks
    a ring once round, ``stats`` is ``po_get_bubblechain_all_stats``, and ``ov`` may be a ``cyclic.HostSuperbubblesAll``,
    which holds its own graph (``graph_res`` is ignored)."""
    if cyclic:
        order = graph_res.node_order() if isinstance(ov, ExactOverlapper) else ov.node_order()
        if superbubbles is None:
            superbubbles = _superbubbles(ov, graph_res, cyclic=True)
        node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains_all(graph_res, min_nodes, len(order))
        return BubbleChains(order, node_chain, node_bubble, edge_chain, table, superbubbles.node_exit, ov.bubblechain_all_stats())
    order = graph_res.node_order()
    if superbubbles is None:
        superbubbles = _superbubbles(ov, graph_res)
    node_chain, node_bubble, edge_chain, table = ov.layout_bubblechains(graph_res, min_nodes, len(order))
    return BubbleChains(order, node_chain, node_bubble, edge_chain, table, superbubbles.node_exit, ov.bubblechain_stats())


def chains_by_component(chains: BubbleChains, components: Components) -> List[List[int]]:
    """Per weakly connected component the chains in it, in chain order: chain ``out[i][j]`` is what `phasm chain` writes as
    ``component{i}.bubblechain{j}`` (its own j follows the iteration order of a Python set)."""
    out = [[] for _ in range(len(components))]
    if len(chains):
        rank = np.zeros(int(chains.node_order.max()) + 1, dtype=np.int64)
        rank[chains.node_order] = np.arange(len(chains.node_order))
        for c, i in enumerate(components.component_of_node[rank[chains.table["first_entrance"]]].tolist()):
            out[i].append(c)
    return out


# ---- the contigs outside the bubble chains (identify_contigs, phasm/assembly_graph.py:655-718) --------------------------------

@dataclass
class Contigs:
    """The contigs of a graph result (``po_layout_contigs``).  ``node_order``: the graph's nodes in the reference's order;
    ``edge_contig`` / ``edge_pos`` (``_lib.NO_NODE`` where there is none): per edge, in the graph's edge order, the contig
    whose path holds it and its 0-based place on that path; ``table``: structured (``first_node``, ``last_node``,
    ``n_nodes``, ``first_edge``, ``length``), one entry per contig: the paths by (rank of the first node, head edge), then
    the one-node contigs by rank (the reference numbers them in the pop order of a queue filled in the iteration order of a
    Python set); ``stats``: ``po_get_contig_stats``; ``edge_ends``: (u, v) of every edge of the graph, [n, 2]."""
    node_order: np.ndarray
    edge_contig: np.ndarray
    edge_pos: np.ndarray
    table: np.ndarray
    stats: dict
    edge_ends: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return len(self.table)

    def edges_of(self, j: int) -> np.ndarray:
        """The indices of the edges of the path of contig ``j``, in path order (none for a one-node contig)."""
        if not hasattr(self, "_edge_group"):
            from ._lib import NO_NODE
            on = np.flatnonzero(self.edge_contig != NO_NODE)
            on = on[np.lexsort((self.edge_pos[on], self.edge_contig[on]))]          # by contig, then by place
            self._edge_group = (on, np.concatenate(([0], np.cumsum(np.bincount(self.edge_contig[on], minlength=len(self))))))
        by, off = self._edge_group
        return by[off[j]:off[j + 1]]

    def path_of(self, j: int) -> List[int]:
        """The node ids of contig ``j`` in path order (a node as often as the path meets it); ``[n]`` for a one-node contig."""
        idx = self.edges_of(j)
        if not len(idx):
            return [int(self.table["first_node"][j])]
        ends = self.edge_ends[idx]
        return [int(ends[0, 0])] + ends[:, 1].astype(np.int64).tolist()


def identify_contigs(ov: ExactOverlapper, graph_res: OverlapResult, min_contig_len: int = 5000, min_nodes: int = 1,
                     exclude=None, cyclic: bool = False) -> Contigs:
    """``po_layout_contigs`` on a graph result of ``ov`` (an edge result, a merged graph or a ``graph_from_edges`` result),
    which stays valid and in HBM.  ``exclude`` None: the nodes of the bubble chains (``min_nodes`` as in ``bubble_chains``),
    built on the device by the same call; else one flag per node, parallel to the node order.  ``cyclic=True``:
    ``po_layout_contigs_all`` instead -- the chains are those of ``bubble_chains(..., cyclic=True)``, ring chains included."""
    order = graph_res.node_order()
    stage = ov.layout_contigs_all if cyclic else ov.layout_contigs
    edge_contig, edge_pos, table = stage(graph_res, min_contig_len, min_nodes, exclude, len(order))
    rows = graph_res.rows()
    ends = np.stack([rows["u"], rows["v"]], axis=1) if len(rows) else np.zeros((0, 2), dtype=np.uint32)
    return Contigs(order, edge_contig, edge_pos, table, ov.contig_stats(), ends)


def contigs_by_component(contigs: Contigs, components: Components) -> List[List[int]]:
    """Per weakly connected component the contigs in it, in contig order: contig ``out[i][j]`` is what `phasm chain` writes as
    ``component{i}.contig{j}`` (its own j follows the pop order of its queue)."""
    out = [[] for _ in range(len(components))]
    if len(contigs):
        rank = np.zeros(int(contigs.node_order.max()) + 1, dtype=np.int64)
        rank[contigs.node_order] = np.arange(len(contigs.node_order))
        for c, i in enumerate(components.component_of_node[rank[contigs.table["first_node"]]].tolist()):
            out[i].append(c)
    return out


def induced_edges(graph_edges: np.ndarray, nodes: Sequence[int]) -> np.ndarray:
    """The indices of the edges of ``g.subgraph(nodes)`` in the order networkx yields them: per node of ``nodes`` (each
    once, at its first place) its out-edges in the graph's edge order, those with both ends among the nodes."""
    e = np.asarray(graph_edges).reshape(-1, 4)
    inside, out = set(), []
    first = [n for n in nodes if not (n in inside or inside.add(n))]
    by = np.argsort(e[:, 0], kind="stable")
    lo = np.searchsorted(e[by, 0], first, side="left")
    hi = np.searchsorted(e[by, 0], first, side="right")
    for a, b in zip(lo.tolist(), hi.tolist()):
        out += [int(i) for i in by[a:b].tolist() if int(e[i, 1]) in inside]
    return np.asarray(out, dtype=np.int64)


@dataclass
class ChainGraph:
    """What ``chain_components`` hands to the writers: the graph file as read (``phasm_amd.io.gfa.GraphFile``) and its
    components; with ``partitions=True`` also the strongly connected components and, per component, the partitions that
    superbubble detection starts with; with ``superbubbles=True`` also the superbubbles of the acyclic partitions (with
    ``cyclic=True`` on top those of all partitions, the cyclic ones included, in ``superbubbles_all``); with
    ``bubblechains=True`` also the bubble chains and, per component, the chains in it (``chains_by_component``); with
    ``contigs=True`` also the contigs outside the chains and, per component, the contigs in it (``contigs_by_component``).
    With ``cyclic=True`` the chains and the contigs build on the superbubbles of all partitions: a circular component is a
    ring chain."""
    graph: object
    components: Components
    sccs: Optional[StrongComponents] = None
    partitions: Optional[List[List[Partition]]] = None
    superbubbles: Optional[Superbubbles] = None
    superbubbles_all: Optional[Superbubbles] = None
    bubblechains: Optional[BubbleChains] = None
    component_chains: Optional[List[List[int]]] = None
    contigs: Optional[Contigs] = None
    component_contigs: Optional[List[List[int]]] = None


def chain_components(path: str, device: Optional[int] = None, partitions: bool = False, superbubbles: bool = False,
                     bubblechains: bool = False, min_nodes: int = 1, contigs: bool = False, min_length: int = 5000,
                     cyclic: bool = False) -> ChainGraph:
    """The start of `phasm chain` on a graph file: ``read_graph_gfa``, one segment per ``S`` line on a fresh handle, the
    graph on the device (``graph_from_edges``) and its weakly connected components; with ``partitions`` also
    ``strongly_connected_components`` and ``superbubble_partitions``; with ``superbubbles`` also ``superbubbles`` (and with
    ``cyclic`` on top ``superbubbles(..., cyclic=True)``: those of all partitions, in ``superbubbles_all``); with
    ``bubblechains`` also ``bubble_chains`` (``min_nodes`` as in ``build_bubblechains``) and ``chains_by_component``; with
    ``contigs`` also ``identify_contigs`` outside those chains (``min_length`` as `phasm chain -l`) and
    ``contigs_by_component``; ``cyclic`` feeds both (``bubble_chains(..., cyclic=True)``, ``identify_contigs(...,
    cyclic=True)``)."""
    from .io import gfa
    with open(path) as f:
        graph = gfa.read_graph_gfa(f)
    ov = ExactOverlapper(device=device)
    try:
        for name, n in zip(graph.names, graph.lengths.tolist()):
            ov.add_segment(name, n)
        res = ov.graph_from_edges(graph.edges, graph.node_order)
        try:
            out = ChainGraph(graph, weakly_connected_components(ov, res))
            if partitions:
                out.sccs = strongly_connected_components(ov, res)
                out.partitions = superbubble_partitions(out.sccs, out.components)
            if superbubbles:
                out.superbubbles = _superbubbles(ov, res)
                if cyclic:
                    out.superbubbles_all = _superbubbles(ov, res, cyclic=True)
            if bubblechains:
                if cyclic and out.superbubbles_all is None:
                    out.superbubbles_all = _superbubbles(ov, res, cyclic=True)
                out.bubblechains = bubble_chains(ov, res, min_nodes, out.superbubbles_all if cyclic else out.superbubbles, cyclic=cyclic)
                out.component_chains = chains_by_component(out.bubblechains, out.components)
            if contigs:
                out.contigs = identify_contigs(ov, res, min_length, min_nodes, cyclic=cyclic)
                out.component_contigs = contigs_by_component(out.contigs, out.components)
            return out
        finally:
            res.free()
    finally:
        ov.close()


def graph_file_bubble_paths(path: str, max_paths: int = 0, device: Optional[int] = None):
    """A graph file by the route of ``chain_components`` -- ``read_graph_gfa``, one segment per ``S`` line on a fresh handle,
    the graph on the device (``graph_from_edges``) -- then ``po_phase_paths``: ``(graph file, phasing.BubblePaths, stats)``.
    The successor order is that of the file's ``E`` lines, as in the graph ``gfa2_reconstruct_assembly_graph`` builds."""
    from .io import gfa
    from .phasing import bubble_paths
    with open(path) as f:
        graph = gfa.read_graph_gfa(f)
    ov = ExactOverlapper(device=device)
    try:
        for name, n in zip(graph.names, graph.lengths.tolist()):
            ov.add_segment(name, n)
        res = ov.graph_from_edges(graph.edges, graph.node_order)
        try:
            return graph, bubble_paths(ov, res, max_paths), ov.paths_stats()
        finally:
            res.free()
    finally:
        ov.close()


def graph_file_device_paths(path: str, max_paths: int = 0, device: Optional[int] = None):
    """``graph_file_bubble_paths`` with the listed paths KEPT on the device: ``(graph file, DevicePaths, stats)``.  The fresh
    handle the graph was put on lives as long as the ``DevicePaths``, whose ``close()`` closes it too."""
    from .io import gfa
    with open(path) as f:
        graph = gfa.read_graph_gfa(f)
    ov = ExactOverlapper(device=device)
    try:
        for name, n in zip(graph.names, graph.lengths.tolist()):
            ov.add_segment(name, n)
        res = ov.graph_from_edges(graph.edges, graph.node_order)
        try:
            paths = ov.phase_paths_resident(res, max_paths)
        finally:
            res.free()
        paths._owned.append(ov)
        return graph, paths, ov.paths_stats()
    except BaseException:
        ov.close()
        raise


def component_gfa2_lines(graph, nodes: Sequence[int], edges: np.ndarray) -> List[str]:
    """What ``gfa2_write_graph`` (phasm/io/gfa.py:281-326) writes for the subgraph of ``nodes`` (in node order) with
    ``edges`` (rows of ``graph.edges``, input order)."""
    from .io import gfa
    out, segments = [gfa.gfa_header()], set()
    for n in nodes:
        seg = int(n) >> 1
        name, length = graph.names[seg], graph.node_length(n)
        if name in segments:
            continue
        segments.add(name)
        out.append(gfa.gfa_line("S", name, length, "*"))
        if seg in graph.fragments:
            reads, prefix = graph.fragments[seg]
            total, cur = sum(prefix), 0
            for k, read in enumerate(reads):
                p = prefix[k] if k < len(prefix) else None
                out.append(gfa.gfa_line("F", name, read, cur, cur + p if p else length, 0, p if p else length - total, "*"))
                if p:
                    cur += p
    for u, v, w, o in np.asarray(edges).reshape(-1, 4).tolist():
        out.append("E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (graph.node_name(u), graph.node_name(v), w, graph.node_length(u), o))
    return out


def component_gfa1_lines(graph, nodes: Sequence[int], edges: np.ndarray) -> List[str]:
    """What ``gfa1_write_graph`` (phasm/io/gfa.py:250-278) writes for the same subgraph."""
    from .io import gfa
    out, segments = [gfa.gfa_header("1.0")], set()
    for n in nodes:
        name = graph.names[int(n) >> 1]
        if name in segments:
            continue
        segments.add(name)
        out.append(gfa.gfa_line("S", name, "*", "LN:i:{}".format(graph.node_length(n))))
    for u, v, _, o in np.asarray(edges).reshape(-1, 4).tolist():
        a, b = graph.node_name(u), graph.node_name(v)
        out.append(gfa.gfa_line("L", a[:-1], a[-1:], b[:-1], b[-1:], str(o) + "M"))
    return out


class _ComponentView:
    """One component with the surface ``write_graphml`` reads."""

    def __init__(self, graph, nodes, edges):
        self.node_order, self.avg_coverage = np.asarray(nodes), None
        self.node_name = graph.node_name
        self._edges = [(graph.node_name(u), graph.node_name(v), w, o) for u, v, w, o in np.asarray(edges).reshape(-1, 4).tolist()]

    def edge_tuples(self):
        return self._edges


def write_component_graphs(out_dir: str, g: ChainGraph, formats: Sequence[str] = ("gfa2",)) -> int:
    """``component{i}.gfa`` and / or ``component{i}.graphml`` for every component, as ``_write_graphs`` writes them
    (assembler.py:215-228, :303-304): ``gfa1`` and ``gfa2`` go to the same name, so with both the later one wins.  Where
    ``g`` carries bubble chains, before each component's own files also ``component{i}.bubblechain{j}.gfa`` / ``.graphml``
    for every chain j of component i with the reference's log line (assembler.py:272-286), and the component's GraphML
    carries the node attribute ``bubblechain`` = j.  Where ``g`` carries contigs, behind the chain files the reference's log
    line and ``component{i}.contig{j}.gfa`` / ``.graphml`` for every contig j of component i -- what ``g.subgraph(path)``
    holds: the nodes of the path in path order, and every edge of the graph with both ends among them --, and the
    component's GraphML carries the edge attribute ``contig`` = j on the edges of the reported paths (assembler.py:288-301).
    Returns the number of components."""
    os.makedirs(out_dir, exist_ok=True)
    comps = g.components

    def write(stem, nodes, edges, marks, edge_marks=None):
        for file_format in formats:
            if file_format.startswith("gfa"):
                lines = (component_gfa1_lines if int(file_format[-1]) == 1 else component_gfa2_lines)(g.graph, nodes, edges)
                with open(os.path.join(out_dir, stem + ".gfa"), "w") as f:
                    f.write("".join(lines))
            else:
                with open(os.path.join(out_dir, stem + ".graphml"), "w") as f:
                    write_graphml(f, _ComponentView(g.graph, nodes, edges), marks, edge_marks)

    for i in range(len(comps)):
        nodes, idx = comps.nodes_of(i).tolist(), comps.edges_of(i)
        edges = g.graph.edges[idx]
        logger.info("Connected component %d with %d nodes and %d edges.", i, len(nodes), len(edges))
        marks = None
        if g.bubblechains is not None:
            marks = {}
            for j, c in enumerate(g.component_chains[i]):
                c_nodes, c_edges = g.bubblechains.nodes_of(c).tolist(), g.graph.edges[g.bubblechains.edges_of(c)]
                logger.info("Found bubblechain #%d with %d nodes and %d edges", j, len(c_nodes), len(c_edges))
                marks.update((g.graph.node_name(n), j) for n in c_nodes)
                write("component%d.bubblechain%d" % (i, j), c_nodes, c_edges, None)
        edge_marks = None
        if g.contigs is not None:
            logger.info("Building contigs not part of a bubble chain...")
            edge_marks, place = {}, {int(e): k for k, e in enumerate(idx.tolist())}
            for j, c in enumerate(g.component_contigs[i]):
                path, seen = g.contigs.path_of(c), set()
                edge_marks.update((place[int(e)], j) for e in g.contigs.edges_of(c).tolist())
                p_nodes = [n for n in path if not (n in seen or seen.add(n))]
                write("component%d.contig%d" % (i, j), p_nodes, g.graph.edges[induced_edges(g.graph.edges, p_nodes)], None)
        write("component%d" % i, nodes, edges, marks, edge_marks)
    return len(comps)
