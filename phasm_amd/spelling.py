"""Spelling: the DNA of paths through a graph file, out of the reads a handle holds.

The reference spells a path with ``AssemblyGraph.sequence_for_path`` (phasm/assembly_graph.py:67-87) over the edges
``node_path_edges`` gives (:99-133): ``get_sequence(u)[:weight]`` per edge, then the whole last node.  ``get_sequence``
(phasm/io/sequences.py:32-65) upper-cases a read and takes the reverse complement for ``-``; a merged node is the concatenation
of ``seq[:prefix_len]`` over its reads, **the whole read where the prefix length is 0 or missing**.

Every path so reduces to PIECES ``(oriented read id, take)``, ``0 <= take <= len(read)``: the sequence is the first ``take``
bytes of each piece's read behind one another, a-z as A-Z.  This module builds the pieces (host control flow, Python slicing
included); ``ExactOverlapper.spell`` turns them into bytes on the device (``po_spell``), ``HostSpeller`` does the same in numpy
for machines without a GPU and for the tests -- it is no fallback of the device call.

Not pinned by anything here: the complement of IUPAC letters (the reads go on the handle in both orientations, whatever wrote
the ``-`` strand decided it), and the line format of the FASTA the reference writes through dinopy."""
from __future__ import annotations

import os
from typing import Iterable, List, Sequence, Tuple

import numpy as np

SPELL_MAX_BYTES = 2**32 - 16

_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32
_IS_ACGT = np.zeros(256, dtype=bool)
_IS_ACGT[[ord(c) for c in "ACGT"]] = True


def spell_arrays(seq_off, piece_read, piece_take) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The three arrays of a spell call as the C ABI takes them (uint64, uint32, uint32); a value that does not fit, or
    piece arrays of two lengths: ValueError."""
    out = []
    for a, dt, what in ((seq_off, np.uint64, "seq_off"), (piece_read, np.uint32, "piece_read"), (piece_take, np.uint32, "piece_take")):
        a = np.asarray(a)
        if a.dtype != dt:
            a = np.asarray(a, dtype=np.int64).reshape(-1) if len(a) else np.zeros(0, dtype=np.int64)
            if len(a) and (int(a.min()) < 0 or int(a.max()) > np.iinfo(dt).max):
                raise ValueError("%s holds a value that is negative or does not fit %s" % (what, np.dtype(dt).name))
        out.append(np.ascontiguousarray(a.reshape(-1), dtype=dt))
    if len(out[0]) < 1:
        raise ValueError("seq_off needs n_seqs + 1 entries")
    if len(out[1]) != len(out[2]):
        raise ValueError("piece_read and piece_take differ in length")
    return out[0], out[1], out[2]


class ReadMap:
    """Oriented read names (``name+`` / ``name-``) -> oriented read ids of a handle, with the lengths of the reads: what
    ``node_pieces`` needs to know of the handle.  ``ReadMap.of(ov)`` reads both from an ``ExactOverlapper`` or a
    ``HostSpeller`` whose reads were added as ``name+``, ``name-`` (ids ``2i``, ``2i + 1`` of FASTA record ``i``)."""

    def __init__(self, names: Sequence[str], lengths: Sequence[int]):
        if len(names) != len(lengths):
            raise ValueError("as many lengths as names")
        self.ids = {name: i for i, name in enumerate(names)}
        self.lengths = [int(x) for x in lengths]

    @classmethod
    def of(cls, ov) -> "ReadMap":
        return cls(ov.ids(), ov.lengths())

    def __getitem__(self, name: str) -> int:
        try:
            return self.ids[name]
        except KeyError:
            raise KeyError("the handle holds no read named %r" % (name,)) from None

    def length(self, rid: int) -> int:
        return self.lengths[rid]


def slice_take(length: int, bound: int) -> int:
    """``len(seq[:bound])`` for a sequence of ``length`` bytes: the three cases of Python slicing."""
    length, bound = int(length), int(bound)
    if bound >= 0:
        return min(bound, length)
    return max(0, length + bound)


def prefix_take(prefix_len, read_len: int) -> int:
    """What a read of a merged node contributes (sequences.py:57-63): ``seq[:prefix_len]`` if the prefix length is truthy,
    else -- a prefix length of 0, or none (the last read) -- the whole read."""
    return slice_take(read_len, prefix_len) if prefix_len else int(read_len)


def node_pieces(gf, node: int, reads_of: ReadMap) -> List[Tuple[int, int]]:
    """The pieces of one node of ``gf`` (an ``io.gfa.GraphFile``): a plain node is its read, whole; a merged node its reads
    under ``prefix_take``.  As many prefix lengths as reads, or too few: ValueError, as the reference raises."""
    node = int(node)
    seg = node >> 1
    if seg not in gf.fragments:
        rid = reads_of[gf.node_name(node)]
        return [(rid, reads_of.length(rid))]
    if node & 1:
        raise ValueError("%s: a merged node exists in forward orientation only" % gf.node_name(node))
    reads, prefixes = gf.fragments[seg]
    if len(reads) != len(prefixes) + 1:
        raise ValueError("merged node %s: %d reads need %d prefix lengths, not %d" % (gf.names[seg], len(reads), len(reads) - 1, len(prefixes)))
    pieces = []
    for k, name in enumerate(reads):
        rid = reads_of[name]
        pieces.append((rid, prefix_take(prefixes[k] if k < len(prefixes) else None, reads_of.length(rid))))
    return pieces


def _edge_weights(gf) -> dict:
    w = getattr(gf, "_spell_weights", None)
    if w is None:
        w = {(int(u), int(v)): int(weight) for u, v, weight, _ in gf.edges.tolist()}
        gf._spell_weights = w
    return w


def path_edges(gf, nodes: Sequence[int]) -> List[Tuple[int, int, int]]:
    """``node_path_edges`` (assembly_graph.py:99-133): the edges (u, v, weight) between consecutive nodes; fewer than two
    nodes or a missing edge: ValueError."""
    nodes = [int(n) for n in nodes]
    if len(nodes) < 2:
        raise ValueError("Not enough nodes to generate a path from")
    weights = _edge_weights(gf)
    edges = []
    for u, v in zip(nodes, nodes[1:]):
        if (u, v) not in weights:
            raise ValueError("Given nodes do not form a path, edge %s not exist" % ((gf.node_name(u), gf.node_name(v)),))
        edges.append((u, v, weights[(u, v)]))
    return edges


def truncate_pieces(pieces: Sequence[Tuple[int, int]], bound: int) -> List[Tuple[int, int]]:
    """``sequence[:bound]`` of the sequence the pieces spell, as pieces: the slice cuts across them.  Every piece stays in
    the list -- one that the cut leaves nothing of has take 0 -- so a node always gives as many pieces as it has reads."""
    left = slice_take(sum(t for _, t in pieces), bound)
    out = []
    for rid, take in pieces:
        t = min(take, left)
        out.append((rid, t))
        left -= t
    return out


def path_pieces(gf, nodes: Sequence[int], reads_of: ReadMap, include_last: bool = True) -> List[Tuple[int, int]]:
    """The pieces of ``sequence_for_path`` over the edges of the node path: per edge (u, v, weight) the sequence OF THE NODE u
    cut at ``[:weight]``, then -- when asked, and when the last node has a length other than 0, which is what the reference's
    ``if include_last and last`` tests -- the whole last node."""
    pieces = []
    for u, _, weight in path_edges(gf, nodes):
        pieces += truncate_pieces(node_pieces(gf, u, reads_of), weight)
    last = int(nodes[-1])
    if include_last and gf.node_length(last):
        pieces += node_pieces(gf, last, reads_of)
    return pieces


def linear_order(gf) -> List[int]:
    """The node order of a graph that is one simple path (every in- and out-degree at most 1, one start, no cycle), or the
    single node of a one-node graph: the graphs on which the ``topological_sort`` the reference uses there is unique.
    Anything else: ValueError that says what is wrong."""
    nodes = [int(n) for n in gf.node_order]
    if not nodes:
        raise ValueError("the graph has no node")
    succ, indeg = {}, dict.fromkeys(nodes, 0)
    for u, v, _, _ in gf.edges.tolist():
        if u in succ:
            raise ValueError("not a simple path: node %s has more than one successor (a fork)" % gf.node_name(u))
        succ[u] = v
        indeg[v] += 1
        if indeg[v] > 1:
            raise ValueError("not a simple path: node %s has more than one predecessor (a fork)" % gf.node_name(v))
    starts = [n for n in nodes if indeg[n] == 0]
    if not starts:
        raise ValueError("not a simple path: every node has a predecessor (a ring)")
    if len(starts) > 1:
        raise ValueError("not a simple path: %d nodes without a predecessor (%s, %s, ...): more than one path" % (
            len(starts), gf.node_name(starts[0]), gf.node_name(starts[1])))
    order = [starts[0]]
    while order[-1] in succ and len(order) <= len(nodes):
        order.append(succ[order[-1]])
    if len(order) != len(nodes):
        raise ValueError("not a simple path: %d of %d nodes lie on a ring beside the path" % (len(nodes) - len(order), len(nodes)))
    return order


def spell_pieces(ov, piece_lists: Iterable[Sequence[Tuple[int, int]]]) -> List[bytes]:
    """Many piece lists in ONE ``spell`` call of ``ov`` (an ``ExactOverlapper`` or a ``HostSpeller``)."""
    seq_off, flat = [0], []
    for pieces in piece_lists:
        flat += pieces
        seq_off.append(len(flat))
    arr = np.asarray(flat, dtype=np.int64).reshape(-1, 2)
    return ov.spell(seq_off, arr[:, 0], arr[:, 1])


def spell_paths(ov, gf, paths: Iterable[Sequence[int]], include_last: bool = True, reads_of: ReadMap = None) -> List[bytes]:
    """The sequences of many node paths of one graph file, in one device call."""
    reads_of = reads_of or ReadMap.of(ov)
    return spell_pieces(ov, [path_pieces(gf, nodes, reads_of, include_last) for nodes in paths])


def contig_pieces(gf, reads_of: ReadMap) -> List[Tuple[int, int]]:
    """What the no-bubble branch of the reference's ``phase`` spells for a graph (phasm/cli/assembler.py:368-383): the node's
    own sequence when there is one node, else the path over the (here unique) topological order."""
    order = linear_order(gf)
    return node_pieces(gf, order[0], reads_of) if len(order) == 1 else path_pieces(gf, order, reads_of, True)


def contig_name(path: str) -> str:
    return os.path.splitext(os.path.basename(path))[0]


class HostSpeller:
    """The ``spell`` contract in numpy over the bytes of every oriented read, modelled on the device's two steps: letters out
    of the 2-bit codes (a byte other than upper-case ACGT has code 0: ``A``), then the exception records with ``pos < take``
    patched in, upper-cased.  For machines without a GPU and for the tests; ``ExactOverlapper.spell`` never calls it."""

    def __init__(self, sequences: Sequence[bytes], ids: Sequence[str] = None):
        self._seqs = [bytes(s) if not isinstance(s, str) else s.encode("latin-1") for s in sequences]
        self._ids = list(ids) if ids is not None else None
        self._len = np.asarray([len(s) for s in self._seqs], dtype=np.int64)
        self._start = np.zeros(len(self._seqs) + 1, dtype=np.int64)
        np.cumsum(self._len, out=self._start[1:])
        self._cat = np.frombuffer(b"".join(self._seqs), dtype=np.uint8)
        self._exc = np.flatnonzero(~_IS_ACGT[self._cat])   # places of the exception records in _cat, ascending
        self._stats = {"n_seqs": 0, "n_pieces": 0, "n_bytes": 0, "n_patched": 0, "device_ms": 0.0}

    def __len__(self) -> int:
        return len(self._seqs)

    def ids(self) -> List[str]:
        if self._ids is None:
            raise ValueError("this HostSpeller was made without read names")
        return self._ids

    def lengths(self) -> np.ndarray:
        return self._len.copy()

    # the two places a broken speller differs (tests/test_spell_oracle.py)
    def _records_end(self, start: np.ndarray, take: np.ndarray, length: np.ndarray) -> np.ndarray:
        """Per piece, the place in _cat behind the last exception record that is patched: pos < take."""
        return start + take

    def _case(self, b: np.ndarray) -> np.ndarray:
        return _UPPER[b]

    def spell(self, seq_off, piece_read, piece_take) -> List[bytes]:
        seq_off, read, take = spell_arrays(seq_off, piece_read, piece_take)
        seq_off, read, take = seq_off.astype(np.int64), read.astype(np.int64), take.astype(np.int64)
        n = len(read)
        if seq_off[0] != 0 or seq_off[-1] != n or np.any(np.diff(seq_off) < 0):
            raise ValueError("spell: seq_off does not run from 0 to n_pieces in ascending order")
        if n and int(read.max()) >= len(self._seqs):
            raise ValueError("spell: a piece names read %d, the speller holds %d" % (int(read.max()), len(self._seqs)))
        if np.any(take > self._len[read]):
            raise ValueError("spell: a piece takes more bytes than its read has")
        total = int(take.sum())
        if total > SPELL_MAX_BYTES:
            raise OverflowError("spell: %d bytes in one call, at most 2^32 - 16" % total)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(take, out=off[1:])
        start = self._start[read]
        src = np.repeat(start - off[:-1], take) + np.arange(total, dtype=np.int64)
        raw = self._cat[src]
        out = np.where(_IS_ACGT[raw], raw, np.uint8(ord("A")))
        # the exception records of every piece
        lo = np.searchsorted(self._exc, start, side="left")
        hi = np.searchsorted(self._exc, self._records_end(start, take, self._len[read]), side="left")
        hi = np.where(take > 0, np.maximum(hi, lo), lo)
        cnt = hi - lo
        n_patched = int(cnt.sum())
        if n_patched:
            first = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(cnt, out=first[1:])
            rec = np.repeat(lo - first[:-1], cnt) + np.arange(n_patched, dtype=np.int64)
            place = self._exc[rec]
            at = place - np.repeat(start, cnt) + np.repeat(off[:-1], cnt)
            ok = at < total
            out[at[ok]] = self._case(self._cat[place[ok]])
        blob = out.tobytes()
        self._stats = {"n_seqs": len(seq_off) - 1, "n_pieces": n, "n_bytes": total, "n_patched": n_patched, "device_ms": 0.0}
        bo = off[seq_off].tolist()
        return [blob[bo[s]:bo[s + 1]] for s in range(len(bo) - 1)]

    def spell_stats(self) -> dict:
        return dict(self._stats)
