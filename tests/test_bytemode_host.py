"""Byte mode (8 bits per base) without a GPU: the oracle premise the GPU byte-mode tests stand on, and the host store's
switch from 2 to 8 bits.

The premise.  The contract compares raw bytes, so its rows depend only on the read lengths and on which substrings are
equal.  A bijection f on byte values keeps both: the rows of [f(s) for s in reads] are the rows of the reads.  With
f = swapcase a read set of upper-case ACGT becomes fully soft-masked (byte mode for every read set with long enough
reads); with f = ACGT -> CATG it stays 2-bit and strand-paired, but every 2-bit code moves.  tests/test_gpu_bytemode.py
checks the HIP rows of the mapped goldens against the golden rows; if the premise were wrong, this file fails first."""
import ctypes

import numpy as np
import pytest

import golden_utils as gu
from oracle import overlap_oracle as oo

SWAPCASE = bytes.maketrans(b"ACGTacgt", b"acgtACGT")
ROTATE = bytes.maketrans(b"ACGT", b"CATG")   # commutes with complementation: comp(f(x)) == f(comp(x))
MAPS = {"swapcase": lambda s: s.swapcase(), "rotate": lambda s: s.translate(ROTATE)}


def test_the_maps_are_bijections_that_commute_with_complement():
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    for name, f in MAPS.items():
        img = f(bytes(range(256)))
        assert len(set(img)) == 256, name
        s = b"ACGTTGCAAGCT"
        assert f(s).translate(comp) == f(s.translate(comp)), name


@pytest.mark.parametrize("name", sorted(MAPS))
def test_brute_force_rows_are_invariant_under_the_map(name):
    f = MAPS[name]
    cases = gu.all_small_cases()
    assert len(cases) > 400
    for case, seqs, m, want in cases:
        got = oo.brute_force([f(s) for s in seqs], m)
        assert np.array_equal(got, want), (name, case)


@pytest.mark.parametrize("ladder", ["ladder_small", "ladder_varlen", "ladder_cfg2_mini"])
def test_c_oracle_rows_are_invariant_under_swapcase(ladder):
    _, seqs, m, want = gu.ladder_case(ladder)
    assert np.array_equal(oo.oracle_overlaps([s.swapcase() for s in seqs], m), want)


# ---- the host store across the switch from 2 to 8 bits per base

def _store_words(ov):
    from phasm_amd import _lib
    lib = _lib.load()
    out = []
    for k in (0, 1):
        ptr = ctypes.c_void_p()
        n = lib.po_debug_store_words(ov._h, k, ctypes.byref(ptr))
        out.append(np.frombuffer(ctypes.string_at(ptr.value, n * 8), dtype=np.uint64).copy() if n else np.zeros(0, np.uint64))
    return out


def unpack_stores(ov, lengths, bits):
    """The reads as the two packed stores hold them (read r in store r & 1, each read on a 16-byte boundary, one zero guard
    word behind it -- append_packed).  At 2 bits an exception byte is code 0 in the words ('A')."""
    stores = _store_words(ov)
    per = 64 // bits
    used = [0, 0]
    reads = []
    for r, n in enumerate(lengths):
        w = stores[r & 1]
        off = (used[r & 1] + 1) & ~1
        nw = (n + per - 1) // per
        assert off + nw + 1 <= len(w), (r, off, nw, len(w))
        assert w[off + nw] == 0, "guard word behind read %d" % r
        words = w[off:off + nw]
        if bits == 8:
            reads.append(words.view(np.uint8)[:n].tobytes())
        else:
            codes = (words[:, None] >> (np.arange(32, dtype=np.uint64) * 2)) & np.uint64(3)
            reads.append(bytes(b"ACGT"[c] for c in codes.reshape(-1)[:n]))
        used[r & 1] = off + nw + 1
    assert used == [len(stores[0]), len(stores[1])], "the stores hold more than the reads"
    return reads


def _as_2bit(s):
    return bytes(c if c in b"ACGT" else ord("A") for c in s)


def _with_bytes(s, positions, byte_values):
    b = bytearray(s)
    for p, v in zip(positions, byte_values):
        b[p] = v
    return bytes(b)


def test_sparse_exceptions_then_a_dense_read_widen_every_read_losslessly():
    from phasm_amd.overlapper import ExactOverlapper
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = []
    for n in (33, 64, 65, 100, 1000, 4097):
        base = acgt[rng.integers(0, 4, size=n)].tobytes()
        for exc in (b"NNNN", b"nacg", b"RYKM", b"a-*t"):
            reads.append(_with_bytes(base, (0, 31, 32, n - 1), exc))   # an exception in the first and last byte of word 0 and 1
        reads.append(base)
    ov = ExactOverlapper()
    for i, s in enumerate(reads):
        ov.add_sequence("r%d" % i, s)
    # still 2 bits per base: the exception bytes are records beside code 0
    assert unpack_stores(ov, [len(s) for s in reads], 2) == [_as_2bit(s) for s in reads]
    dense = bytes(rng.choice(np.frombuffer(b"acgtN", dtype=np.uint8), size=500))
    ov.add_sequence("dense", dense)
    reads.append(dense)
    # every read held so far was re-encoded (materialize: codes, then the exception records on top) at 8 bits
    got = unpack_stores(ov, [len(s) for s in reads], 8)
    for i, (g, s) in enumerate(zip(got, reads)):
        assert g == s, "read %d (%d bytes) changed when the store widened" % (i, len(s))
    # reads added after the switch go straight to 8 bits
    ov.add_sequence("after", b"ACGTNacgt" * 7)
    reads.append(b"ACGTNacgt" * 7)
    assert unpack_stores(ov, [len(s) for s in reads], 8) == reads
    assert ov.lengths().tolist() == [len(s) for s in reads]
    ov.close()


@pytest.mark.parametrize("n", [16, 17, 63, 64, 1000, 4096])
def test_exception_threshold_is_len_over_64_plus_16(n):
    """append_packed keeps a read at 2 bits while it carries at most n / 64 + 16 bytes outside upper-case ACGT: a read of
    16 bases stays 2-bit even when every base is lower case, one of 17 does not."""
    from phasm_amd.overlapper import ExactOverlapper
    rng = np.random.default_rng(n)
    limit = n // 64 + 16
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()
    checks = [(k, bits) for k, bits in ((limit, 2), (limit + 1, 8)) if k <= n]
    assert checks == ([(16, 2)] if n == 16 else [(limit, 2), (limit + 1, 8)])
    for k, bits in checks:
        pos = sorted(rng.choice(n, size=k, replace=False).tolist())
        s = _with_bytes(base, pos, b"n" * k)
        ov = ExactOverlapper()
        ov.add_sequence("pre", b"ACGTACGTAC")      # (a read ahead of it: the switch must carry it along)
        ov.add_sequence("r", s)
        got = unpack_stores(ov, [10, n], bits)
        assert got == ([b"ACGTACGTAC", _as_2bit(s)] if bits == 2 else [b"ACGTACGTAC", s]), (n, k, bits)
        ov.close()
