"""GFA2 line emitter for the overlap file -- the wire format between ``phasm overlap`` and
``phasm layout`` / ``phasm phase``.

Mirrors the two helpers the reference's overlap command uses
(/root/reference/phasm/io/gfa.py:230-231 ``gfa_line`` and :234-240 ``gfa_header``): a line is
its fields joined by tabs plus a newline; the header is ``H\\tVN:z:2.0`` (no ``TS`` tag on this
path).  ``write_edges`` is the bulk form for the 24-byte row array: byte-identical to writing
``gfa_line("E", "*", a, b, astart, aend, bstart, bend, "*")`` per row
(phasm/cli/assembler.py:46-48).
"""
from __future__ import annotations

from typing import BinaryIO, Optional, Sequence, TextIO, Union

import numpy as np


def gfa_line(*args) -> str:
    return "\t".join(map(str, args)) + "\n"


def gfa_header(version: str = "2.0", trace_spacing: Optional[int] = None) -> str:
    parts = ["H", "VN:z:{}".format(version)]
    if trace_spacing:
        parts.append("TS:i:{:d}".format(trace_spacing))
    return gfa_line(*parts)


def write_edges(out: Union[TextIO, BinaryIO], rows: np.ndarray, ids: Sequence[str], chunk: int = 1 << 18) -> int:
    """Write one ``E`` line per row of the structured row array; returns the line count."""
    ids_arr = np.asarray(ids, dtype=object)
    n = len(rows)
    binary = "b" in getattr(out, "mode", "") or isinstance(out, (bytes, bytearray))
    for lo in range(0, n, chunk):
        r = rows[lo:lo + chunk]
        a = ids_arr[r["a_idx"]]
        b = ids_arr[r["b_idx"]]
        lines = ["E\t*\t%s\t%s\t%d\t%d\t%d\t%d\t*\n" % t
                 for t in zip(a, b, r["astart"].tolist(), r["aend"].tolist(),
                              r["bstart"].tolist(), r["bend"].tolist())]
        blob = "".join(lines)
        out.write(blob.encode("utf-8") if binary else blob)
    return n


# ---- reading side: what `phasm layout` takes from the overlap file ----------------------------

def _gfa_pos_to_int(pos: str) -> int:
    """/root/reference/phasm/io/gfa.py:65-69: a position may carry the GFA2 end marker ``$``."""
    return int(pos[:-1]) if pos.endswith("$") else int(pos)


def gfa2_parse_segment(line: str):
    """``S <id> <length> <sequence|*>`` -> (id, length); mirrors gfa2_segment_to_read (gfa.py:33-46)."""
    if not line.startswith("S"):
        raise ValueError("Given GFA2 line is not a segment.")
    parts = line.strip().split("\t")
    _ = parts[3]                       # the reference indexes the sequence field (IndexError if absent)
    return parts[1].strip(), int(parts[2])


def gfa2_parse_edge(line: str):
    """``E * <sid1> <sid2> <b1> <e1> <b2> <e2> <alignment>`` -> (sid1, sid2, arange, brange);
    mirrors gfa2_parse_edge (gfa.py:72-87)."""
    if not line.startswith("E"):
        raise ValueError("Given GFA2 line is not an edge.")
    parts = line.strip().split("\t")
    _ = parts[8]
    arange = tuple(map(_gfa_pos_to_int, parts[4:6]))
    brange = tuple(map(_gfa_pos_to_int, parts[6:8]))
    return parts[2].strip(), parts[3].strip(), arange, brange


def read_gfa2_rows(lines):
    """Pure-Python reading of a GFA2 text the way ``phasm layout`` does (assembler.py:56-60, 96-98):
    -> (names, lengths, rows) with node index 2*i for ``name+`` and 2*i+1 for ``name-``.  The bulk path
    is the native ``po_add_gfa``; this is the readable counterpart the tests compare it with."""
    lines = list(lines)
    order, length = {}, []
    for ln in lines:
        if ln.startswith("S"):
            sid, n = gfa2_parse_segment(ln)
            if sid in order:
                length[order[sid]] = n      # dict semantics: the last S line of a name wins (gfa.py:109)
            else:
                order[sid] = len(length)
                length.append(n)
    rows = []
    for ln in lines:
        if ln.startswith("E"):
            s1, s2, ar, br = gfa2_parse_edge(ln)
            nodes = []
            for sid in (s1, s2):
                if sid[-1:] not in ("+", "-"):
                    raise ValueError("segment reference without strand: %r" % sid)
                nodes.append(2 * order[sid[:-1]] + (sid[-1] == "-"))   # KeyError like reads[sid[:-1]] (gfa.py:97-98)
            rows.append((nodes[0], nodes[1], ar[0], ar[1], br[0], br[1]))
    names = list(order)
    return names, np.asarray(length, dtype=np.int64), np.asarray(rows, dtype=np.int64).reshape(-1, 6)


# ---- reading side: what `phasm chain` takes from the graph file `phasm layout` wrote --------------

class GraphFile:
    """A graph file as `phasm chain` rebuilds it (gfa2_parse_segments_with_fragments and gfa2_reconstruct_assembly_graph,
    phasm/io/gfa.py:112-227 of the reference).  Segment i of ``names`` / ``lengths`` (file order) has the nodes 2i (``+``)
    and 2i+1 (``-``); a segment with ``F`` lines is a merged node, which exists as ``+`` only: ``fragments[i]`` holds its
    reads (as written, strand sign included) and its prefix lengths.  ``edges`` is an int64 array (u, v, weight,
    overlap_len) in the order the graph first saw each edge, ``node_order`` the nodes in the graph's order."""

    def __init__(self, names, lengths, fragments, edges, node_order):
        self.names, self.lengths, self.fragments, self.edges, self.node_order = names, lengths, fragments, edges, node_order

    def node_name(self, n: int) -> str:
        n = int(n)
        return self.names[n >> 1] + "+-"[n & 1]

    def node_length(self, n: int) -> int:
        return int(self.lengths[int(n) >> 1])


def read_graph_gfa(lines) -> GraphFile:
    """``S``, ``F`` and ``E`` lines of a graph file -> GraphFile.  Segments keep their file order (the last ``S`` line of a
    name wins and keeps the first one's place); the fragments of a merged segment are sorted by segment start, its prefix
    lengths are the fragment lengths with the last dropped.  An edge has weight ``astart - bstart`` and overlap_len
    ``max(aend - astart, bend - bstart)``; positions may carry a trailing ``$``; a second ``E`` line for the same (u, v)
    overwrites the attributes and keeps the position.  Node order: first appearance in the ``E`` lines, u before v; then,
    in ``S``-line order, the ``+`` node of every segment of which neither orientation got an edge.  An ``E`` line that
    names an unknown node (the ``-`` of a merged segment included) raises KeyError, as the reference's lookup does."""
    lines = list(lines)
    index, seg_line, frags = {}, [], {}
    for ln in lines:
        if not ln.startswith("S") and not ln.startswith("F"):
            continue
        parts = ln.strip().split("\t")
        kind, name = parts[0].strip(), parts[1].strip()
        if kind == "S":
            if name in index:
                seg_line[index[name]] = ln
            else:
                index[name] = len(seg_line)
                seg_line.append(ln)
        if kind == "F":
            seg_range = tuple(map(_gfa_pos_to_int, parts[3:5]))
            frag_range = tuple(map(_gfa_pos_to_int, parts[5:7]))
            frags.setdefault(name, []).append((seg_range[0], parts[2].strip(), frag_range[1] - frag_range[0]))
    names = list(index)
    lengths = np.asarray([gfa2_parse_segment(ln)[1] for ln in seg_line], dtype=np.int64)
    fragments, nodes = {}, {}
    for name, i in index.items():
        nodes[name + "+"] = 2 * i
        if name in frags:
            ordered = sorted(frags[name], key=lambda f: f[0])          # (stable, like the reference's sorted)
            fragments[i] = ([f[1] for f in ordered], [f[2] for f in ordered][:-1])
        else:
            nodes[name + "-"] = 2 * i + 1
    place, edges, order, seen = {}, [], [], set()
    for ln in lines:
        if ln.startswith("E"):
            s1, s2, ar, br = gfa2_parse_edge(ln)
            u, v = nodes[s1], nodes[s2]
            attrs = [u, v, ar[0] - br[0], max(ar[1] - ar[0], br[1] - br[0])]
            for n in (u, v):
                if n not in seen:
                    seen.add(n)
                    order.append(n)
            if (u, v) in place:
                edges[place[(u, v)]] = attrs
            else:
                place[(u, v)] = len(edges)
                edges.append(attrs)
    for i in range(len(names)):
        if 2 * i not in seen and 2 * i + 1 not in seen:
            order.append(2 * i)
    return GraphFile(names, lengths, fragments, np.asarray(edges, dtype=np.int64).reshape(-1, 4), order)
