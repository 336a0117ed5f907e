"""What the tests of po_spell over every form of the device read store share (tests/test_gpu_spell_stores.py and the CPU tests
beside it): the reference, which is plain Python slicing of the bytes that were added; the read sets -- 28 record lengths
around the 32-base and 8-byte word edges, and reads that hold the bytes next to the range the upper-casing tests for --;
the calls -- the sweep (output-offset residue x read x take), the whole-reads read-back, a random call --; and what the
library's statistics must say about them.  Nothing here goes through HostSpeller or numpy arithmetic on the bytes."""
import bisect

import numpy as np

import spell_utils as su

EDGE_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129)
LONG_TAKES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
SWEEP_SIZE = (23_328, 69_984, 922_896)          # sequences, pieces, bytes of sweep_call over the 56 edge reads
# the bytes on both sides of a-z and A-Z, bytes >= 0x80 (the low seven bits of 0xE1 and 0xFA are `a` and `z`), the ends of
# the two ranges themselves, N and n.  `A` is no exception record in a 2-bit store -- it is there for the 8-bit one.
ODD_BYTES = b"@[`{\x80\xe1\xfa\xff" + b"azAZNn"
ODD_POSITIONS = (0, 7, 8, 31, 32, -1)


def plain_spell(reads, seq_off, piece_read, piece_take):
    """THE reference: per sequence the first `take` bytes of each piece's read behind one another, ASCII a-z as A-Z
    (`bytes.upper()` touches nothing else, which is the contract of spell.hip.h)."""
    seq_off = [int(x) for x in seq_off]
    pr, pt = [int(x) for x in piece_read], [int(x) for x in piece_take]
    return [b"".join([reads[pr[p]][:pt[p]] for p in range(seq_off[s], seq_off[s + 1])]).upper() for s in range(len(seq_off) - 1)]


def edge_records(seed=7):
    """(name, bytes) of forward records of the 28 EDGE_LENGTHS: random ACGT; every third non-empty record carries bytes from
    `Nnacgt` at position 0, at len - 1, and at 31, 32 and 33 (clamped to len - 1)."""
    rng = np.random.default_rng(seed)
    recs, k = [], 0
    for ln in EDGE_LENGTHS:
        s = bytearray(b"ACGT"[i] for i in rng.integers(0, 4, size=ln))
        if ln:
            if k % 3 == 0:
                for pos in sorted({0, ln - 1, min(31, ln - 1), min(32, ln - 1), min(33, ln - 1)}):
                    s[pos] = b"Nnacgt"[int(rng.integers(6))]
            k += 1
        recs.append(("e%d" % ln, bytes(s)))
    return recs


def edge_reads(seed=7):
    """The 56 strand-paired reads of edge_records."""
    return [s for _, s in su.oriented(edge_records(seed))]


def acgt_only(recs):
    """The records with every byte other than ACGT replaced (a-z upper-cased, then A): what the parallel FASTA ingest takes."""
    table = bytes(c if c in b"ACGT" else ord("A") for c in range(256))
    return [(n, s.upper().translate(table)) for n, s in recs]


def dense_read(n=70):
    """One read with more bytes other than ACGT than n / 64 + 16: it moves a handle to 8 bits per base."""
    return bytes(b"ACGTNnacgtRy"[(5 * i) % 12] for i in range(n))


def _call(piece_lists):
    seq_off, pr, pt = [0], [], []
    for pieces in piece_lists:
        for r, t in pieces:
            pr.append(r)
            pt.append(t)
        seq_off.append(len(pr))
    return np.asarray(seq_off, dtype=np.uint64), np.asarray(pr, dtype=np.uint32), np.asarray(pt, dtype=np.uint32)


def sweep_takes(length):
    if length <= 65:
        return list(range(length + 1))
    return sorted(set(LONG_TAKES) | {length - d for d in (33, 32, 31, 17, 16, 15, 1, 0)})


def sweep_call(reads, residues=range(16)):
    """One sequence [(filler, o), (r, t), (filler + 1, 5)] per output-offset residue o, read r and take t of sweep_takes: the
    product that decides which of the one to three words a fetch loads and how the chunk is shifted into place.  The filler
    is the (first) read of 129 bases, filler + 1 its partner (a set that ends with the filler: the read before it)."""
    filler = next(i for i, s in enumerate(reads) if len(s) == 129)
    tail = filler + 1 if filler + 1 < len(reads) else filler - 1
    assert len(reads[tail]) >= 5
    return _call([[(filler, o), (r, t), (tail, 5)] for o in residues for r in range(len(reads)) for t in sweep_takes(len(reads[r]))])


def whole_reads_call(reads):
    """One sequence per read with take == len: the read-back of the store, the last read of each store and the empty reads
    included."""
    return _call([[(r, len(s))] for r, s in enumerate(reads)])


def random_call(reads, seed, n_seqs=300, max_pieces=6):
    """Sequences of 0 .. max_pieces pieces over random reads with takes 0 .. len, both ends included now and then."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_seqs):
        pieces = []
        for _ in range(int(rng.integers(0, max_pieces + 1))):
            r = int(rng.integers(len(reads)))
            ln = len(reads[r])
            pieces.append((r, int(rng.choice([0, ln, int(rng.integers(0, ln + 1))]))))
        out.append(pieces)
    return _call(out)


def odd_bytes_reads(seed=19):
    """-> (set a, set b) of UNPAIRED reads (no reverse complement of these bytes is defined or needed).
    (a): 14 reads of 200 to 300 random ACGT bases; read i holds ODD_BYTES[(i + j) % 14] at ODD_POSITIONS[j], so every byte
    stands once at each of the positions 0, 7, 8, 31, 32 and len - 1.  Six bytes per read (five exception records where one of
    them is `A`): fewer than len / 64 + 16, the handle stays at 2 bits and the bytes go through k_spell_patch / spell_upper.
    (b): (a) and one read of 240 bytes that cycles through ODD_BYTES and `C` (15 bytes: every one of them at every position
    within an 8-byte word), dense enough to widen the handle: the same bytes through spell_upper8.
    po_add_sequence refuses no byte value (a sequence is a pointer and a length), so none is left out."""
    rng = np.random.default_rng(seed)
    a = []
    for i in range(len(ODD_BYTES)):
        s = bytearray(b"ACGT"[k] for k in rng.integers(0, 4, size=int(rng.integers(200, 301))))
        for j, pos in enumerate(ODD_POSITIONS):
            s[pos] = ODD_BYTES[(i + j) % len(ODD_BYTES)]
        a.append(bytes(s))
    cycle = ODD_BYTES + b"C"
    return a, a + [bytes(cycle[i % len(cycle)] for i in range(240))]


def exception_positions(read):
    return [i for i, c in enumerate(read) if c not in b"ACGT"]


def expected_bits(reads):
    """8 once a read holds more bytes other than ACGT than len / 64 + 16 (append_packed), else 2."""
    return 8 if any(len(exception_positions(s)) > len(s) // 64 + 16 for s in reads) else 2


def count_patched(reads, piece_read, piece_take, bits):
    """n_patched of a call: the exception records below the take, over all pieces; an 8-bit store has no records."""
    if bits != 2:
        return 0
    exc = [exception_positions(s) for s in reads]
    return sum(bisect.bisect_left(exc[int(r)], int(t)) for r, t in zip(piece_read, piece_take))


def store_words(reads, parity, bits):
    """64-bit words of host store `parity` (append_packed: a read starts on a 16-byte boundary, one guard word behind it)."""
    per, size = 64 // bits, 0
    for s in reads[parity::2]:
        size = ((size + 1) & ~1) + (len(s) + per - 1) // per + 1
    return size


def upload_bytes(reads, bits, half):
    """What the plain upload moves to the device: the per-read tables, the exception records of a 2-bit store, store 0 and
    -- unless the odd reads are rebuilt on the device (`half`) -- store 1."""
    n = len(reads)
    n_exc = sum(len(exception_positions(s)) for s in reads) if bits == 2 else 0
    total = n * 12 + (n + 1) * 4 + ((n + 1) * 4 + n_exc * 5 if n_exc else 0) + 8 * store_words(reads, 0, bits)
    return total if half else total + 8 * store_words(reads, 1, bits)


def first_difference(got, want):
    """None when the two lists of bytes are equal, else a short text that names the first sequence that differs (a plain
    `==` on 23 000 sequences is as exact; its failure report is not readable)."""
    if got == want:
        return None
    if len(got) != len(want):
        return "%d sequences, expected %d" % (len(got), len(want))
    s = next(i for i in range(len(want)) if got[i] != want[i])
    return "sequence %d of %d: got %r, expected %r" % (s, len(want), got[s][:200], want[s][:200])
