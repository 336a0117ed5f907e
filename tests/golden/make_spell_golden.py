#!/usr/bin/env python3
"""Generate tests/golden/spell_cases.npz by EXECUTING the reference's own spelling.

Runs only where the reference checkout is present; the output (inputs and recorded values only) is committed.

    AssemblyGraph.sequence_for_path                                  phasm/assembly_graph.py:67-87
    AssemblyGraph.node_path_edges                                    phasm/assembly_graph.py:99-133
    SequenceSource.get_sequence / _get_merged_reads_sequence         phasm/io/sequences.py:32-65

run UNMODIFIED, on graphs that the reference's ``gfa2_parse_segments_with_fragments`` and ``gfa2_reconstruct_assembly_graph``
build from the GFA text kept in the file.  Stand-in code of ours, and why:
  * the installed networkx (3.x) takes ``add_edge(u, v, **attr)`` where the reference passes the attribute dict by position:
    ``Graph`` below is the reference's AssemblyGraph with that one method adapted, and the parser builds it;
  * ``phasm.io.sequences`` imports dinopy, which is not installed: an empty module of that name stands in ``sys.modules``
    (only ``FastaSource`` uses it).  ``DictSource`` is a ``SequenceSource`` whose ``_get_sequence`` serves the reads from a dict,
    upper-cased, a ``-`` strand through ``phasm_amd.io.fasta.reverse_complement``;
  * ``node_path_edges`` ends by letting ``next()`` raise StopIteration inside the generator, which Python 3.7+ turns into a
    RuntimeError: ``edges_of`` draws the edges one by one and takes that RuntimeError as the end.
What this leaves UNPINNED: the complement of IUPAC letters (ours, not dinopy's -- the exception bytes here are N, n and
lower-case acgt only, on which every complement table agrees), and the line format of the FASTA writer.

The expected PIECES are what ``phasm_amd.spelling.path_pieces`` gives, recorded after ``HostSpeller`` over them has given the
reference's bytes: they pin the piece builder against a regression, the bytes pin it against the reference.

``orders``: the node order of a graph that is one simple path is ``networkx.topological_sort`` of the reference's graph (what
the no-bubble branch of phasm/cli/assembler.py:368-383 spells); a ring, a fork and two paths are errors of OUR contract
(``linear_order``): on the last two a topological order exists and is not unique.

    --time    instead of writing the file, print what the reference's sequence_for_path takes on a path of 50 000 nodes"""
import io
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")
sys.modules.setdefault("dinopy", types.ModuleType("dinopy"))

import networkx  # noqa: E402
import numpy as np  # noqa: E402

import phasm.assembly_graph as ag  # noqa: E402  (reference)
import phasm.io.gfa as rgfa  # noqa: E402  (reference)
from phasm.alignments import MergedReads, Read  # noqa: E402  (reference)
from phasm.io.sequences import SequenceSource  # noqa: E402  (reference)

import spell_utils as su  # noqa: E402
from phasm_amd import spelling  # noqa: E402
from phasm_amd.io.fasta import reverse_complement  # noqa: E402

assert ag.AssemblyGraph.sequence_for_path.__code__.co_filename.startswith("/root/reference/")
assert SequenceSource.get_sequence.__code__.co_filename.startswith("/root/reference/")


class Graph(ag.AssemblyGraph):
    def add_edge(self, u, v, attr_dict=None, **attr):
        super().add_edge(u, v, **dict(attr_dict or {}, **attr))


rgfa.AssemblyGraph = Graph


class DictSource(SequenceSource):
    def __init__(self, seqs):
        super().__init__()
        self.seqs = seqs

    def _get_sequence(self, read):
        seq = self.seqs[read.id].upper()
        return reverse_complement(seq) if read.orientation == "-" else seq


def edges_of(g, nodes):
    out, it = [], g.node_path_edges(nodes, data=True)
    while True:
        try:
            out.append(next(it))
        except StopIteration:
            return out
        except RuntimeError as e:
            if isinstance(e.__cause__, StopIteration):
                return out
            raise


# ---- the reads ------------------------------------------------------------------------------------------------------------

rng = random.Random(20261020)


def dna(n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def with_bytes(seq, marks):
    s = list(seq)
    for pos, b in marks.items():
        s[pos] = b
    return "".join(s)


READS = [("one", dna(1)), ("two", dna(2))]
READS += [("s%d" % k, dna(k + 1)) for k in range(48)]            # s_k has k + 1 bases
READS[2 + 7] = ("s7", with_bytes(READS[2 + 7][1], {3: "a"}))     # (a few lower-case letters among the short reads)
READS[2 + 20] = ("s20", with_bytes(READS[2 + 20][1], {0: "g", 20: "t"}))
READS += [("L200", dna(200)), ("L2049", dna(2049)), ("f1", dna(90)), ("f2", dna(70)), ("f3", dna(33)), ("f4", dna(64)), ("f5", dna(120))]
# exception records: at position 0 and len - 1, lower case, N and n, next to a word boundary (32, 33)
READS += [("X70", with_bytes(dna(70), {0: "N", 5: "a", 16: "n", 31: "c", 32: "N", 33: "g", 69: "t"})),
          ("allN", "N" * 12),                                      # (12 <= 12 / 64 + 16: stays a 2-bit read)
          ("nn5", "nNnNn")]
# the wide set: one read dense enough in non-ACGT for 8 bits per base (41 > 60 / 64 + 16), one with the other exception bytes
DENSE = [("D60", with_bytes(dna(60), {i: "Nn"[i & 1] for i in range(0, 41)})),
         ("D40", with_bytes(dna(40), {1: "a", 2: "c", 3: "g", 4: "t", 8: "N", 15: "n", 16: "N", 17: "a", 39: "n"}))]
LEN = {n: len(s) for n, s in READS + DENSE}


def S(name, length=None):
    return "S\t%s\t%d\t*\n" % (name, LEN[name] if length is None else length)


def E(u, v, weight, bstart=0):
    # weight = astart - bstart; the ends only feed overlap_len
    return "E\t*\t%s\t%s\t%d\t%d\t%d\t%d\t*\n" % (u, v, weight + bstart, weight + bstart + 5, bstart, bstart + 5)


def merged(name, length, frags):
    """S and F lines of a merged segment: frags = [(oriented read, prefix length or None for the last)]."""
    text, at = "S\t%s\t%d\t*\n" % (name, length), 0
    for read, prefix in frags:
        n = prefix if prefix is not None else 7          # (the last fragment's length is dropped by the parser)
        text += "F\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (name, read, at, at + n, n)
        at += n
    return text


def star(u, weights, targets, declare=True):
    """u with one edge per weight, each to a target of its own; the paths [u, target], without the last node."""
    text = (S(u[:-1]) if declare else "") + "".join(S(t) for t in targets[:len(weights)])
    text += "".join(E(u, t + "+", w) for w, t in zip(weights, targets))
    return text, [[u, t + "+"] for w, t in zip(weights, targets)]


CASES = []


def case(name, gfa, paths, include_last, reads="main", **more):
    if isinstance(include_last, bool):
        include_last = [include_last] * len(paths)
    CASES.append(dict(name=name, reads=reads, gfa="H\tVN:z:2.0\n" + gfa, paths=paths, include_last=[bool(x) for x in include_last], **more))


SMALL = ["s%d" % k for k in range(48)]
# take values around the chunk and word sizes, the clipping weight, the negative weights; empty sequences first, in the middle, last
for big in ("L200", "L2049"):
    L = LEN[big]
    w = [0, 1, 15, 16, 17, 31, 32, 33, 0, 63, 64, 65, L, L - 1, L + 50, -5, -(L - 1), -L, -(L + 3)]
    for sign in "+-":
        text, paths = star(big + sign, w, SMALL)
        case("takes_%s%s" % (big, sign), text, paths, False)
text, paths = star("L2049+", [1023, 1024, 1025, 2047, 2048, 2049], SMALL)
case("takes_L2049_deep", text, paths, False)
# exception records: at take - 1 (in) and at take (out), position 0 and len - 1, both strands (store 0 and store 1)
for sign in "+-":
    w = [0, 1, 2, 5, 6, 16, 17, 31, 32, 33, 34, 35, 69, 70, 80, -1, -38]
    text, paths = star("X70" + sign, w, SMALL)
    case("exceptions_X70" + sign, text, paths, False)
text, paths = star("allN+", [0, 1, 11, 12], SMALL)
case("no_acgt_at_all", text + S("nn5") + E("allN-", "nn5-", 12), paths + [["allN-", "nn5-"]], [False] * 4 + [True])
# 40 and more pieces of take 1 and 0: one 16-byte chunk covers many pieces
w = [1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1] * 2 + [1, 0, 1, 1]
nodes = ["s%d+" % k for k in range(3, 3 + len(w) + 1)]
case("ones_and_zeros", "".join(S(n[:-1]) for n in nodes) + "".join(E(u, v, x) for u, v, x in zip(nodes, nodes[1:], w)), [nodes], True)
# pieces at every output offset mod 16: the weights 1 .. 16 put them at the triangular numbers
w = list(range(1, 18))
nodes = ["s%d+" % k for k in range(20, 20 + len(w) + 1)]
assert {sum(w[:k]) % 16 for k in range(len(w))} == set(range(16))
case("every_residue", "".join(S(n[:-1]) for n in nodes) + "".join(E(u, v, x) for u, v, x in zip(nodes, nodes[1:], w)), [nodes], True)
# a read of one base; + and - of one read in one path
case("one_base", S("one") + S("two") + E("one+", "two+", 1) + E("one-", "two-", 1) + E("two+", "one-", 5),
     [["one+", "two+"], ["one-", "two-"], ["two+", "one-"], ["one+", "two+"]], [True, True, True, False])
case("both_strands_of_a_read", S("L200") + S("s9") + E("L200+", "L200-", 37) + E("L200-", "s9+", 200) + E("s9+", "L200+", 3),
     [["L200+", "L200-"], ["L200+", "L200-", "s9+", "L200+"]], [True, True])
# merged nodes: 1, 2 and 5 fragments, a prefix length of 0 in the middle, cut inside the first, a middle and the last
# fragment and at a boundary; as the last node; a self-loop
M5 = [("f1+", 40), ("f2-", 25), ("f3+", 0), ("f4-", 64), ("f5+", None)]        # 40 + 25 + 33 + 64 + 120 = 282 bytes
M = merged("m1", 50, [("s30-", None)]) + merged("m2", 60, [("f2+", 30), ("f3-", None)]) + merged("m5", 282, M5)
w = [0, 1, 39, 40, 41, 64, 65, 66, 97, 98, 99, 161, 162, 163, 281, 282, 300, -1, -120, -121, -282, -283]
text, paths = star("m5+", w, SMALL, declare=False)
case("merged_cut", M + text, paths, False)
case("merged_nodes", M + S("s9") + S("L200") + E("s9+", "m5+", 4) + E("m5+", "m1+", 100) + E("m1+", "m2+", 31) + E("m2+", "m2+", 45)
     + E("m2+", "L200-", 63) + E("L200-", "m1+", 1),
     [["s9+", "m5+"], ["s9+", "m5+", "m1+", "m2+"], ["m2+", "m2+"], ["m2+", "m2+", "m2+", "L200-", "m1+"], ["m1+", "m2+"]],
     [True, True, True, True, False])
# a node's own sequence (a graph of one node)
case("single_plain_node", S("L200"), [["L200+"]], True, node_only=True)
case("single_merged_node", merged("m5", 282, M5), [["m5+"]], True, node_only=True)
# a declared length of 0 makes the last node falsy: the reference's `if include_last and last` leaves it out
case("last_node_of_length_0", S("s9") + S("s4", 0) + E("s9+", "s4+", 6), [["s9+", "s4+"]], True)
# errors on both sides
case("mismatch_one_prefix_too_many", M + S("s9") + E("m2+", "s9+", 10), [["m2+", "s9+"]], True, mutate=[["m2", 1]], error="ValueError")
case("mismatch_one_prefix_too_few", M + S("s9") + E("m5+", "s9+", 10), [["m5+", "s9+"]], True, mutate=[["m5", -1]], error="ValueError")
case("one_node_is_no_path", S("s9") + S("s4") + E("s9+", "s4+", 6), [["s9+"]], True, error="ValueError")
case("missing_edge", S("s9") + S("s4") + E("s9+", "s4+", 6), [["s4+", "s9+"]], True, error="ValueError")
case("no_sequences", S("s9"), [], True)
# the wide read set: the dense reads themselves, next to reads of the main set
for sign in "+-":
    w = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 41, 59, 60, 99, -3]
    text, paths = star("D60" + sign, w, SMALL)
    case("dense_D60" + sign, text, paths, False, reads="wide")
case("dense_path", S("D40") + S("D60") + S("X70") + S("s9") + E("D40+", "D60-", 19) + E("D60-", "X70+", 33) + E("X70+", "D40-", 34) + E("D40-", "s9+", 40),
     [["D40+", "D60-", "X70+", "D40-", "s9+"]], True, reads="wide")

ORDERS = []
chain = ["s%d" % k for k in (5, 9, 2, 30, 11, 7)]
lines = [E(u + "+", v + "+", 2) for u, v in zip(chain, chain[1:])]
lines = [lines[i] for i in (3, 0, 4, 2, 1)]
ORDERS.append(dict(name="path_in_shuffled_line_order", gfa="".join(S(n) for n in sorted(chain)) + "".join(lines)))
ORDERS.append(dict(name="single_node", gfa=merged("m5", 282, M5)))
ORDERS.append(dict(name="ring", gfa="".join(S(n) for n in chain[:3]) + E("s5+", "s9+", 1) + E("s9+", "s2+", 1) + E("s2+", "s5+", 1), error="ValueError"))
ORDERS.append(dict(name="fork", gfa="".join(S(n) for n in chain[:3]) + E("s5+", "s9+", 1) + E("s5+", "s2+", 1), error="ValueError"))
ORDERS.append(dict(name="join", gfa="".join(S(n) for n in chain[:3]) + E("s5+", "s2+", 1) + E("s9+", "s2+", 1), error="ValueError"))
ORDERS.append(dict(name="two_paths", gfa="".join(S(n) for n in chain[:4]) + E("s5+", "s9+", 1) + E("s2+", "s30+", 1), error="ValueError"))
ORDERS.append(dict(name="path_beside_a_ring", gfa="".join(S(n) for n in chain[:4]) + E("s5+", "s9+", 1) + E("s2+", "s30+", 1) + E("s30+", "s2+", 1),
                   error="ValueError"))


# ---- the reference ----------------------------------------------------------------------------------------------------------

def reference_graph(text, seqs, mutate=()):
    segments = rgfa.gfa2_parse_segments_with_fragments(io.StringIO(text))
    orig = {name: Read(name, len(s)) for name, s in seqs.items()}
    g = rgfa.gfa2_reconstruct_assembly_graph(io.StringIO(text), segments, orig)
    g.sequence_src = DictSource(seqs)
    nodes = {str(n): n for n in g}
    for seg, delta in mutate:
        n = nodes[seg + "+"]
        assert isinstance(n, MergedReads)
        if delta > 0:
            n.prefix_lengths.append(3)
        else:
            n.prefix_lengths.pop()
    return g, nodes


def main():
    seqs = {w: {n: s.encode("latin-1") for n, s in (READS if w == "main" else READS + DENSE)} for w in ("main", "wide")}
    doc = {"reads": READS, "dense": DENSE, "cases": CASES, "orders": ORDERS}
    su._GOLDEN[:] = [doc]                                  # (spell_utils serves the read sets of the file being made)
    speller = {w: su.host_speller(w) for w in ("main", "wide")}
    maps = {w: spelling.ReadMap.of(speller[w]) for w in ("main", "wide")}
    n_paths = n_bytes = 0
    for c in CASES:
        g, nodes = reference_graph(c["gfa"], seqs[c["reads"]], c.get("mutate", ()))
        c.setdefault("error", "")
        want = []
        try:
            for names, last in zip(c["paths"], c["include_last"]):
                if c.get("node_only"):
                    want.append(g.get_sequence(nodes[names[0]]))
                else:
                    want.append(g.sequence_for_path(edges_of(g, [nodes[n] for n in names]), include_last=last))
            assert not c["error"], c["name"] + ": the reference raised nothing"
        except ValueError:
            assert c["error"] == "ValueError", c["name"]
            try:
                su.pieces_of(c, maps[c["reads"]])
            except ValueError:
                c["pieces"], c["bytes"] = [], []
                continue
            raise AssertionError(c["name"] + ": the piece builder raised nothing")
        pieces = su.pieces_of(c, maps[c["reads"]])
        for w in ("main", "wide") if c["reads"] == "main" else ("wide",):
            got = speller[w].spell(*su.call_arrays(pieces))
            assert got == want, "%s on %s: HostSpeller differs from the reference" % (c["name"], w)
        c["pieces"] = [[list(p) for p in ps] for ps in pieces]
        c["bytes"] = [b.decode("latin-1") for b in want]
        n_paths += len(want)
        n_bytes += sum(len(b) for b in want)
    for o in ORDERS:
        o.setdefault("error", "")
        g, _ = reference_graph(o["gfa"], seqs["main"])
        gf = su.graph_of(o)
        if o["error"]:
            o["order"] = []
            try:
                spelling.linear_order(gf)
            except ValueError:
                continue
            raise AssertionError(o["name"] + ": linear_order raised nothing")
        o["order"] = [str(n) for n in networkx.topological_sort(g)]
        assert [gf.node_name(n) for n in spelling.linear_order(gf)] == o["order"], o["name"]
    # what the cases promise
    takes = {t for c in CASES for ps in c["pieces"] for _, t in ps}
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 199, 200, 2048, 2049} <= takes
    ones = next(c for c in CASES if c["name"] == "ones_and_zeros")["pieces"][0]
    assert len(ones) >= 40 and {t for _, t in ones[:-1]} == {0, 1}
    blob = json.dumps(doc, sort_keys=True).encode("utf-8")
    out = os.path.join(HERE, "spell_cases.npz")
    np.savez_compressed(out, meta=np.frombuffer(blob, dtype=np.uint8))
    print("%d cases (%d paths, %d bytes), %d orders -> %s (%d bytes)" % (len(CASES), n_paths, n_bytes, len(ORDERS), out, os.path.getsize(out)))


def time_reference(n=50_000, read_len=1500):
    """--time: the reference's sequence_for_path over a path of `n` plain nodes with weights around 1 000 (the shape of a
    config-2 contig; with the cache warm the cost does not depend on the length of the reads), on this host core."""
    import time
    r = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = {"t%d" % i: letters[r.integers(0, 4, read_len)].tobytes() for i in range(n)}
    weights = np.clip(np.rint(r.normal(1000, 150, n)), 0, read_len).astype(int).tolist()
    text = "".join("S\tt%d\t%d\t*\n" % (i, read_len) for i in range(n))
    text += "".join(E("t%d+" % i, "t%d+" % (i + 1), weights[i]) for i in range(n - 1))
    g, nodes = reference_graph(text, seqs)
    edges = edges_of(g, [nodes["t%d+" % i] for i in range(n)])
    cold = time.perf_counter()
    want = g.sequence_for_path(edges)
    cold = time.perf_counter() - cold
    best = min(timed(lambda: g.sequence_for_path(edges)) for _ in range(5))
    print("reference sequence_for_path, %d edges, %d bytes: %.1f ms with a cold cache (upper-casing every read), %.1f ms warm (best of 5)" % (
        len(edges), len(want), 1e3 * cold, 1e3 * best))


def timed(f):
    import time
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


if __name__ == "__main__":
    if "--time" in sys.argv:
        time_reference()
    else:
        main()
