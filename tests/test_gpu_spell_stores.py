"""po_spell on every form of the device read store.  Spelling is the byte-for-byte read-back of the
packed reads in HBM, so each test brings a handle's store into one state -- copied in full, half copied and rebuilt by
k_revcomp_store, left by the streamed step or by its overflow fallback, assembled from shard pieces, grown, widened to 8 bits,
ingested from FASTA, born in poisoned buffers -- names in an assertion the statistics that show the state was reached, and
compares what the device spells with plain Python slicing of the bytes that were added (tests/spell_store_utils.py).  Every
comparison is byte equality; every call is a valid one."""
import numpy as np
import pytest

import checker as ck
import golden_utils as gu
import spell_store_utils as ssu
import spell_utils as su
from oracle import overlap_oracle as oo   # row helpers only
from phasm_amd.overlapper import ExactOverlapper
from test_gpu_streamed import _nested_reads, _with_exceptions

pytestmark = pytest.mark.gpu


def handle(reads, strand_names=False):
    ov = ExactOverlapper()
    for i, s in enumerate(reads):
        ov.add_sequence("r%d%s" % (i // 2, "+-"[i & 1]) if strand_names else "r%d" % i, s)
    return ov


def spelled(ov, reads, call, bits, label):
    """One device call against plain slicing, with the statistics of the call; -> the device's bytes."""
    seq_off, pr, pt = call
    want = ssu.plain_spell(reads, seq_off, pr, pt)
    got = ov.spell(seq_off, pr, pt)
    assert ssu.first_difference(got, want) is None, "%s: %s" % (label, ssu.first_difference(got, want))
    st = ov.spell_stats()
    assert (st["n_seqs"], st["n_pieces"], st["n_bytes"], st["n_patched"]) == (
        len(want), len(pr), sum(map(len, want)), ssu.count_patched(reads, pr, pt, bits)), label
    return got


def assert_store_spells(ov, reads, label, sweep=False, seed=1):
    """The store of `ov` holds `reads`: the whole-reads read-back, a random call with takes 0 .. len and -- on the edge set --
    the sweep equal plain slicing, and spell_stats() agree in n_seqs, n_pieces, n_bytes and n_patched (the exception records
    below the take, counted here on the host).  -> the device's bytes of the calls, for tests that compare two states."""
    bits = ssu.expected_bits(reads)
    out = [spelled(ov, reads, ssu.whole_reads_call(reads), bits, label + ", whole reads")]
    assert ov.spell_stats()["n_bytes"] == sum(len(s) for s in reads)
    out.append(spelled(ov, reads, ssu.random_call(reads, seed), bits, label + ", random call"))
    if sweep:
        out.append(spelled(ov, reads, ssu.sweep_call(reads), bits, label + ", sweep"))
        if len(reads) == 56:
            assert tuple(ov.spell_stats()[k] for k in ("n_seqs", "n_pieces", "n_bytes")) == ssu.SWEEP_SIZE
    return out


def store_stats(ov, m=30):
    """stats() of a resident overlap call on the store as it is (a handle that is not dirty uploads nothing): `paired` and
    `bits_per_base` are set by an overlap call, `upload_bytes` by the upload that made the store."""
    res = ov.overlaps_result(m)
    res.free()
    st = ov.stats()
    assert st["streamed"] == 0
    return st


def streamed_call(ov, seqs, m, label):
    """po_overlaps_to_host on a dirty handle under PHASM_STREAM=1: the streamed step, with the oracle's rows."""
    res = ov.overlaps_to_host_result(m)
    st = ov.stats()
    got = oo.sort_rows(oo.struct_to_rows(res.rows_view()))
    res.free()
    assert st["streamed"] == 1 and st["paired"] == 1 and st["bits_per_base"] == 2, (label, st)
    ck.assert_same_rows(got, ck.oracle_overlaps(seqs, m), seqs, m, label)
    return st


# ---- 1 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [False, True], ids=["", "poisoned"])
def test_sweep_on_both_encodings(poison, monkeypatch):
    """Offset residue x read x take on the 2-bit store (half copied, store 1 rebuilt on the device, records patched) and on
    the same reads behind one dense read (8 bits); again on handles whose fresh device buffers start as 0xA5."""
    if poison:
        monkeypatch.setenv("PHASM_POISON", "0xA5")
    edge = ssu.edge_reads()
    for reads, bits in ((edge, 2), (edge + [ssu.dense_read()], 8)):
        ov = handle(reads)
        try:
            assert_store_spells(ov, reads, "%d bits" % bits, sweep=True)
            assert (ov.spell_stats()["n_patched"] > 0) == (bits == 2)
            small = spelled(ov, reads, ssu.random_call(reads, 2, n_seqs=3), bits, "a small call in the buffers of the sweep")
            assert small == spelled(ov, reads, ssu.random_call(reads, 2, n_seqs=3), bits, "again")
            st = store_stats(ov)
            assert st["bits_per_base"] == bits and st["paired"] == (bits == 2) and st["n_reads"] == len(reads)
            assert st["upload_bytes"] == ssu.upload_bytes(reads, bits, half=bits == 2)   # 2 bits: only store 0 travelled
            assert_store_spells(ov, reads, "%d bits, after an overlap call" % bits, sweep=True)
        finally:
            ov.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1], ids=["records", "bytes"])
def test_odd_bytes(which):
    """@ [ ` { 0x80 0xE1 0xFA 0xFF, a z A Z N n at positions 0, 7, 8, 31, 32 and len - 1: as exception records (spell_upper)
    and, behind one dense read, in the words of an 8-bit store (spell_upper8)."""
    reads = ssu.odd_bytes_reads()[which]
    bits = (2, 8)[which]
    ov = handle(reads)
    try:
        got = assert_store_spells(ov, reads, "odd bytes, %d bits" % bits)[0]
        assert got == [s.upper() for s in reads]
        st = store_stats(ov)
        assert st["paired"] == 0 and st["bits_per_base"] == bits and st["upload_bytes"] == ssu.upload_bytes(reads, bits, half=False)
    finally:
        ov.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------

def test_unpaired_and_odd_count_stores():
    """Stores that are copied in full, both of them, and go through k_paired_check: reads that are no strand pairs (an odd
    number of them), reads over ACGTNacgt, and strand pairs of which one strand holds an N the other lacks."""
    rng = np.random.default_rng(31337)
    genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=5000))
    reads = [genome[int(s):int(s) + int(l)] for s, l in zip(rng.integers(0, 4000, size=41), rng.integers(60, 900, size=41))]
    alpha = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)
    g8 = alpha[rng.integers(0, len(alpha), size=4000)].tobytes()
    reads8 = [g8[int(s):int(s) + int(l)] for s, l in zip(rng.integers(0, 3000, size=37), rng.integers(40, 700, size=37))]
    broken = _nested_reads(9, 10, 2000, 100, 500)
    broken[4] = broken[4][:50] + b"N" + broken[4][51:]
    sparse = [bytes(s) for s in reads[:40]]                     # an even number, no pairs, a few records: 2 bits
    sparse[3] = sparse[3][:31] + b"n" + sparse[3][32:]
    sparse[38] = b"N" + sparse[38][1:-1] + b"t"
    for label, seqs, bits in (("41 genome reads", reads, 2), ("ACGTNacgt reads", reads8, 8), ("N on one strand", broken, 2),
                              ("40 reads with records", sparse, 2)):
        ov = handle(seqs)
        try:
            assert_store_spells(ov, seqs, label)
            st = store_stats(ov)
            assert st["paired"] == 0 and st["bits_per_base"] == bits == ssu.expected_bits(seqs), (label, st)
            assert st["upload_bytes"] == ssu.upload_bytes(seqs, bits, half=False), label
        finally:
            ov.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------

def test_shortcut_off(monkeypatch):
    """The edge set with the half upload off (PHASM_FULL_UPLOAD: both stores copied, pairing checked on the device) and with
    the strand mirror off (PHASM_NO_MIRROR: store 1 still rebuilt, the calls unpaired): the bytes of the plain handle."""
    reads = ssu.edge_reads()
    got = {}
    for switch in ("", "PHASM_FULL_UPLOAD", "PHASM_NO_MIRROR"):
        if switch:
            monkeypatch.setenv(switch, "1")
        ov = handle(reads)
        try:
            got[switch] = assert_store_spells(ov, reads, switch or "plain", sweep=True)
            st = store_stats(ov)
            assert st["bits_per_base"] == 2 and st["paired"] == (switch != "PHASM_NO_MIRROR"), (switch, st)
            assert st["upload_bytes"] == ssu.upload_bytes(reads, 2, half=switch != "PHASM_FULL_UPLOAD"), (switch, st)
        finally:
            ov.close()
            if switch:
                monkeypatch.delenv(switch)
    assert got["PHASM_FULL_UPLOAD"] == got[""] and got["PHASM_NO_MIRROR"] == got[""]


# ---- 5 ------------------------------------------------------------------------------------------------------------------

def streamed_sets():
    """(label, index, min_length, reads, sweep): strand pairs with exception records, the edge set, and the tiny / empty-read
    sets of test_streamed_step_with_empty_and_tiny_reads, one of them at ("wide", 160): k_scatter_lead wrote five words."""
    rng = np.random.default_rng(61)
    base = _nested_reads(3, 30, 1500, 40, 400)
    tiny = [b"", b"", b"ACG", b"CGT", b"A", b"T"]
    mid = [b"ACGTTGCA" * 5 + b"G", (b"ACGTTGCA" * 5 + b"G").translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]]
    return [("exception records", "narrow", 33, _with_exceptions(_nested_reads(100, 60, 5000, 60, 1200), rng, 24), False),
            ("edge set", "narrow", 30, ssu.edge_reads(), True),
            ("tiny reads in the middle", "narrow", 30, base[:20] + tiny + base[20:], False),
            ("tiny reads last, with records", "narrow", 1, _with_exceptions(base, rng, 10) + tiny, False),
            ("tiny reads at both ends", "wide", 64, tiny[:2] + base + tiny[:2], False),
            ("short reads, five lead words", "wide", 160, base[:10] + mid + tiny + base[10:] + mid, False)]


@pytest.mark.parametrize("cuts", ["", "300,700", "100,200,300,400,500,600,700,800,900"])
def test_after_a_streamed_step(cuts, monkeypatch):
    """The store the streamed step leaves: first words scattered ahead, pieces landed on the upload stream, k_revcomp_store
    per piece, the records of the odd reads cleared out of the codes.  Twice per handle."""
    monkeypatch.setenv("PHASM_STREAM", "1")
    if cuts:
        monkeypatch.setenv("PHASM_STREAM_CUTS", cuts)
    n_wide = 0
    for label, index, m, seqs, sweep in streamed_sets():
        monkeypatch.setenv("PHASM_INDEX", index)
        ov = handle(seqs)
        try:
            for call in (1, 2):
                what = "%s, cuts %r, streamed call %d" % (label, cuts, call)
                st = streamed_call(ov, seqs, m, what)
                n_wide += st["wide_index"]
                assert_store_spells(ov, seqs, what, sweep=sweep, seed=call)
                ov.invalidate()
        finally:
            ov.close()
    assert n_wide == 4


# ---- 6 ------------------------------------------------------------------------------------------------------------------

def test_after_the_overflow_fallback(monkeypatch):
    """A streamed attempt that overflowed its deferred list ("a piece may be missing on the device") and fell back to the
    chunked form: the store must be whole again before anything reads it."""
    monkeypatch.setenv("PHASM_STREAM", "1")
    monkeypatch.setenv("PHASM_STREAM_CUTS", "250,500,750")
    monkeypatch.setenv("PHASM_DEFER_CAP", "3")
    rng = np.random.default_rng(7)
    seqs = _with_exceptions(_nested_reads(77, 120, 5000, 40, 1200), rng, 12)
    m = 35
    want = ck.oracle_overlaps(seqs, m)
    ov = handle(seqs)
    try:
        res = ov.overlaps_to_host_result(m)
        st = ov.stats()
        assert st["streamed"] == 0 and st["n_deferred"] > 3 and st["paired"] == 1 and st["bits_per_base"] == 2, st
        ck.assert_same_rows(oo.sort_rows(oo.struct_to_rows(res.rows_view())), want, seqs, m, "overflow fallback")
        res.free()
        assert_store_spells(ov, seqs, "after the overflow fallback")
        monkeypatch.delenv("PHASM_DEFER_CAP")
        ov.invalidate()
        streamed_call(ov, seqs, m, "streamed after the overflow")
        assert ov.stats()["n_deferred"] > 3
        assert_store_spells(ov, seqs, "streamed after the overflow", seed=2)
    finally:
        ov.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [1, 2])
def test_assembled_store(parts):
    """Store 0 put together from the pieces of three shards (whole, and in two parts each), store 1 rebuilt behind them: one
    GPU plays every rank, and the first thing that reads the assembled store is the spell call."""
    import torch
    nshards = 3
    _, seqs, m, want = gu.ladder_case("ladder_varlen")
    ov = ExactOverlapper(device=0)
    try:
        for i, s in enumerate(seqs):
            ov.add_sequence("r%d" % i, s)
        sizes = [[ov.upload_piece_part(k, nshards, q, parts) for q in range(parts)] for k in range(nshards)]
        assert all(ok for row in sizes for ok, _ in row)
        assert sum(n for row in sizes for _, n in row) == ssu.store_words(seqs, 0, 2)   # the pieces tile store 0
        slot = max(n for row in sizes for _, n in row) + 1
        buf = torch.full((parts * nshards * slot,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for q in range(parts):
            for k in range(nshards):
                ok, n = ov.upload_piece_part(k, nshards, q, parts, buf.data_ptr() + 8 * (q * nshards + k) * slot, slot)
                assert ok and n == sizes[k][q][1]
        ov.upload_assemble(buf.data_ptr(), slot, nshards, parts)
        uploaded = ov.stats()["upload_bytes"]
        assert_store_spells(ov, seqs, "assembled from %d x %d pieces" % (nshards, parts))
        st = store_stats(ov, m)
        # (what THIS rank moved: the per-read tables and the pieces, never store 1)
        assert st["paired"] == 1 and st["bits_per_base"] == 2 and st["upload_bytes"] == uploaded <= ssu.upload_bytes(seqs, 2, half=True)
        res = ov.overlaps_result(m)
        ck.assert_same_rows(oo.sort_rows(oo.struct_to_rows(res.rows())), want, seqs, m, "assembled store")
        res.free()
    finally:
        ov.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["resident", "streamed"])
def test_a_handle_that_changes_between_spells(first, monkeypatch):
    """One handle: spell; ten more pairs (new offsets, a larger store 0, so store 1 moves); one unpaired read (both stores
    copied in full); one dense read (every read re-packed at 8 bits, the exception records dropped); the first call again."""
    monkeypatch.setenv("PHASM_STREAM", "1" if first == "streamed" else "0")
    monkeypatch.setenv("PHASM_STREAM_CUTS", "300,700")
    rng = np.random.default_rng(404)
    seqs = _with_exceptions(_nested_reads(41, 40, 4000, 60, 900), rng, 20)
    more = _with_exceptions(_nested_reads(42, 10, 4000, 33, 700), rng, 6)
    m = 40

    def settle(label):
        if first == "streamed":
            streamed_call(ov, seqs, m, label)
    ov = handle(seqs)
    try:
        settle("the first store")
        first_call = ssu.random_call(seqs, 9)
        first_bytes = spelled(ov, seqs, first_call, 2, "first call")
        assert_store_spells(ov, seqs, "the first store")
        st = store_stats(ov, m)
        assert st["paired"] == 1 and st["bits_per_base"] == 2
        before = sum(len(s) for s in seqs)
        spelled(ov, seqs, ssu.whole_reads_call(seqs), 2, "the first store, whole reads")
        assert ov.spell_stats()["n_bytes"] == before
        # grows
        for i, s in enumerate(more):
            ov.add_sequence("more%d" % i, s)
        seqs = seqs + more
        settle("ten more pairs")
        assert_store_spells(ov, seqs, "ten more pairs")
        spelled(ov, seqs, ssu.whole_reads_call(seqs), 2, "ten more pairs, whole reads")
        assert ov.spell_stats()["n_bytes"] == sum(len(s) for s in seqs) > before
        st = store_stats(ov, m)
        assert st["paired"] == 1 and st["bits_per_base"] == 2 and st["n_reads"] == len(seqs)
        if first == "resident":
            assert st["upload_bytes"] == ssu.upload_bytes(seqs, 2, half=True)
        assert spelled(ov, seqs, first_call, 2, "first call on the grown store") == first_bytes
        # one unpaired read: an odd number of reads, nothing is rebuilt on the device
        seqs = seqs + [b"ACGTTGCAAG" * 7 + b"n"]
        ov.add_sequence("single", seqs[-1])
        assert_store_spells(ov, seqs, "one unpaired read")
        st = store_stats(ov, m)
        assert st["paired"] == 0 and st["bits_per_base"] == 2 and st["upload_bytes"] == ssu.upload_bytes(seqs, 2, half=False), st
        assert ov.spell_stats()["n_patched"] > 0
        # a dense read: 8 bits
        seqs = seqs + [ssu.dense_read(300)]
        ov.add_sequence("dense", seqs[-1])
        assert ssu.expected_bits(seqs) == 8
        assert_store_spells(ov, seqs, "widened to 8 bits")
        assert ov.spell_stats()["n_patched"] == 0
        st = store_stats(ov, m)
        assert st["paired"] == 0 and st["bits_per_base"] == 8 and st["upload_bytes"] == ssu.upload_bytes(seqs, 8, half=False), st
        assert spelled(ov, seqs, first_call, 8, "first call on the widened store") == first_bytes
    finally:
        ov.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------

def test_interleaved_with_the_other_users_of_the_handle():
    """spell; rows resident; phase_index on them; spell; layout_edges; spell -- the calls share the host landing zone, the
    pinned scalars, d_scalars and the layout events.  The bytes are equal each time, the rows the golden's before and after."""
    _, seqs, m, want = gu.ladder_case("ladder_varlen")
    ov = handle(seqs, strand_names=True)            # (po_layout_edges wants the names of `phasm overlap`)
    try:
        a = assert_store_spells(ov, seqs, "before any other call")
        res = ov.overlaps_result(m)
        st = ov.stats()
        assert st["paired"] == 1 and st["bits_per_base"] == 2 and st["streamed"] == 0 and st["n_rows"] == len(want)
        assert st["upload_bytes"] == ssu.upload_bytes(seqs, 2, half=True)
        ck.assert_same_rows(oo.sort_rows(oo.struct_to_rows(res.rows())), want, seqs, m, "rows before")
        index = ov.phase_index(res)
        off, entries = ov.phase_index_entries(index)
        b = assert_store_spells(ov, seqs, "after phase_index")
        edges, removed = ov.layout_edges(res)
        n_edges = len(edges)
        c = assert_store_spells(ov, seqs, "after layout_edges")
        assert a == b == c
        ck.assert_same_rows(oo.sort_rows(oo.struct_to_rows(res.rows())), want, seqs, m, "rows after")
        off2, entries2 = ov.phase_index_entries(index)
        assert np.array_equal(off, off2) and np.array_equal(entries, entries2) and len(edges) == n_edges > 0
        for r in (edges, index, res):
            r.free()
    finally:
        ov.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("both_strands", [True, False])
def test_fasta_ingest(both_strands, tmp_path, monkeypatch):
    """po_add_fasta of the edge records, cut into seven ranges: as they are (bytes other than ACGT: record by record) and as
    pure ACGT (the parallel ingest, into host stores that start as 0xA5), spelled against the records themselves."""
    monkeypatch.setenv("PHASM_FASTA_RANGES", "7")
    monkeypatch.setenv("PHASM_POISON_HOST", "1")
    recs = ssu.edge_records()
    for label, records in (("records", recs), ("acgt", ssu.acgt_only(recs))):
        path = tmp_path / (label + ".fasta")
        path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in records))
        reads = [s for _, s in (su.oriented(records) if both_strands else records)]
        ov = ExactOverlapper()
        try:
            assert ov.add_fasta(str(path), both_strands=both_strands) == len(records)
            assert ov.lengths().tolist() == [len(s) for s in reads]
            assert_store_spells(ov, reads, "FASTA %s, both_strands %s" % (label, both_strands), sweep=True)
            st = store_stats(ov)
            assert st["bits_per_base"] == 2 and st["paired"] == both_strands and st["n_reads"] == len(reads)
            assert st["upload_bytes"] == ssu.upload_bytes(reads, 2, half=both_strands)
        finally:
            ov.close()
