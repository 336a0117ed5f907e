"""What the spelling tests share (tests/golden/spell_cases.npz, made by tests/golden/make_spell_golden.py from the reference's
own sequence_for_path, node_path_edges and get_sequence): the golden as Python objects, the handles its read sets go on, and
the calls of a case.

The golden: ``reads`` -- (name, bytes) of the FASTA records of the "main" read set; ``dense`` -- the records the "wide" set has
behind them, one of which holds enough bytes other than ACGT to move a handle to 8 bits per base; ``cases`` -- per case a
graph file as GFA text, node paths by name with their ``include_last``, and either the expected pieces and bytes per path or
the error both sides raise; ``orders`` -- graph files with the node order ``linear_order`` must give, or the error.
Bytes travel as latin-1 strings."""
import io
import json
import os

import numpy as np

from phasm_amd import spelling
from phasm_amd.io import gfa
from phasm_amd.io.fasta import reverse_complement

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spell_cases.npz")
_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        with np.load(GOLDEN_FILE) as z:
            _GOLDEN.append(json.loads(z["meta"].tobytes().decode("utf-8")))
    return _GOLDEN[0]


def records(which):
    """(name, bytes) of the FASTA records of a read set: "main", or "wide" = main and the dense records behind them."""
    g = load_golden()
    recs = [(n, s.encode("latin-1")) for n, s in g["reads"]]
    if which == "wide":
        recs += [(n, s.encode("latin-1")) for n, s in g["dense"]]
    return recs


def oriented(recs):
    """The oriented reads of FASTA records as `phasm overlap` adds them: (name+, x), (name-, reverse complement of x)."""
    out = []
    for name, seq in recs:
        out.append((name + "+", seq))
        out.append((name + "-", reverse_complement(seq)))
    return out


def host_speller(which, cls=spelling.HostSpeller):
    reads = oriented(records(which))
    return cls([s for _, s in reads], ids=[n for n, _ in reads])


def add_reads(ov, which):
    for name, seq in oriented(records(which)):
        ov.add_sequence(name, seq)
    return ov


def cases(which=None):
    """The cases that run on a read set: every "main" case runs on "wide" too (the same ids, the same bytes)."""
    return [c for c in load_golden()["cases"] if which is None or c["reads"] == "main" or c["reads"] == which]


def graph_of(case):
    gf = gfa.read_graph_gfa(io.StringIO(case["gfa"]))
    for seg, delta in case.get("mutate", []):      # a merged node with one prefix length too many (+1) or too few (-1)
        i = gf.names.index(seg)
        reads, prefixes = gf.fragments[i]
        gf.fragments[i] = (reads, prefixes + [3] if delta > 0 else prefixes[:-1])
    return gf


def node_id(gf, name):
    return 2 * gf.names.index(name[:-1]) + (name[-1] == "-")


def pieces_of(case, reads_of, node_pieces=None):
    """The piece list of every path of a case (a path of ONE node stands for the node's own sequence)."""
    gf = graph_of(case)
    out = []
    for names, last in zip(case["paths"], case["include_last"]):
        nodes = [node_id(gf, n) for n in names]
        if case.get("node_only"):
            out.append(spelling.node_pieces(gf, nodes[0], reads_of))
        else:
            out.append(spelling.path_pieces(gf, nodes, reads_of, bool(last)))
    return out


def expected_bytes(case):
    return [s.encode("latin-1") for s in case["bytes"]]


def call_arrays(piece_lists):
    """(seq_off, piece_read, piece_take) of one spell call over the given piece lists."""
    seq_off, flat = [0], []
    for p in piece_lists:
        flat += [tuple(x) for x in p]
        seq_off.append(len(flat))
    arr = np.asarray(flat, dtype=np.int64).reshape(-1, 2)
    return np.asarray(seq_off, dtype=np.uint64), arr[:, 0].astype(np.uint32), arr[:, 1].astype(np.uint32)


def good_cases(which):
    return [c for c in cases(which) if not c["error"]]


def big_call(n_pieces=600_000, seed=11):
    """One call past a capped grid (524 288 lanes) in chunks and in pieces: ~300 oriented reads from ``synth``, a few of them
    with exception records, `n_pieces` pieces with takes 0 .. 33 (about 10 MB of output) in 1 000 sequences, empty ones among
    them.  -> (oriented reads [(name, bytes)], seq_off, piece_read, piece_take)"""
    from phasm_amd import synth
    cfg = synth.SynthConfig(n_reads=150, read_len=2000, genome_len=20000, seed=seed, len_sd=600.0, len_min=200, len_max=4000)
    recs = synth.generate_reads(cfg)
    rng = np.random.default_rng(seed)
    for i in range(0, len(recs), 10):               # N, n and lower case into every tenth read, the first and last byte included
        s = bytearray(recs[i][1])
        for pos in [0, len(s) - 1] + rng.integers(0, len(s), 6).tolist():
            s[pos] = rng.choice(list(b"Nnacgt"))
        recs[i] = (recs[i][0], bytes(s))
    reads = oriented(recs)
    lens = np.asarray([len(s) for _, s in reads], dtype=np.int64)
    piece_read = rng.integers(0, len(reads), n_pieces).astype(np.uint32)
    piece_take = np.minimum(rng.integers(0, 34, n_pieces), lens[piece_read]).astype(np.uint32)
    seq_off = np.sort(np.concatenate([[0, 0, n_pieces, n_pieces], rng.integers(0, n_pieces + 1, 997)])).astype(np.uint64)
    return reads, seq_off, piece_read, piece_take
