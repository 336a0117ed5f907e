"""Byte mode on the GPU: every kernel's BITS = 8 instantiation (W = 8 bases per word, 512-base scan tiles, the K-mer
masked below min_length 8, the wide index from min_length 15, a's words in LDS up to 56 712 bases) against the goldens and
the oracle.

The goldens become byte-mode goldens through a bijection on byte values (tests/test_bytemode_host.py states and checks
the premise): swapcase turns every read set into a soft-masked one -- 8 bits per base wherever the reads are long enough
for the lower case to exceed the exception budget, 2 bits with exception records on every base elsewhere; ACGT -> CATG
keeps 2 bits and the strand pairing but moves every 2-bit code (a real 'A' becomes 'C', exception bytes stay on code 0)."""
import os

import numpy as np
import pytest

import checker as ck
import golden_utils as gu
from oracle import overlap_oracle as oo   # row helpers only: the oracle runs in the checker process
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

ROTATE = bytes.maketrans(b"ACGT", b"CATG")
MAPS = {"swapcase": lambda s: s.swapcase(), "rotate": lambda s: s.translate(ROTATE)}
COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def revcomp(s):
    return s.translate(COMP)[::-1]


def expected_bits(seqs):
    """8 once some read carries more than len / 64 + 16 bytes outside upper-case ACGT (append_packed), else 2."""
    return 8 if any(sum(c not in b"ACGT" for c in s) > len(s) // 64 + 16 for s in seqs) else 2


def _sorted(arr):
    return oo.sort_rows(oo.struct_to_rows(arr))


def handle(seqs):
    ov = ExactOverlapper()
    for i, s in enumerate(seqs):
        ov.add_sequence("r%d" % i, s)
    return ov


def whole(ov, m):
    return _sorted(ov.overlaps_array(m)), ov.stats()


def sharded(ov, m, n=3):
    parts = [ov.overlaps_shard_array(m, k, n) for k in range(n)]
    return _sorted(np.concatenate(parts)), ov.stats()


def to_host(ov, m):
    res = ov.overlaps_to_host_result(m)
    got = _sorted(res.rows_view())
    res.free()
    return got, ov.stats()


def cands_expanded(ov, m, n=3):
    """The multi-GPU exchange form: per-shard compacted candidates, concatenated, expanded by po_expand."""
    import torch
    from phasm_amd.dist import _result_to_tensor
    dev = torch.device("cuda", 0)
    parts = []
    for k in range(n):
        res = ov.candidates_result(m, k, n)
        parts.append(_result_to_tensor(res, 4, dev))
        res.free()
    merged = torch.cat(parts, dim=0).contiguous()
    res = ov.expand_result(merged.data_ptr(), merged.shape[0])
    got = _sorted(res.rows())
    res.free()
    return got, ov.stats()


FORMS = {"whole": whole, "3 shards": sharded, "to_host 3 chunks": to_host}


def check_forms(seqs, m, want, ctx, forms=FORMS):
    ov = handle(seqs)
    bits = set()
    try:
        for fname, form in forms.items():
            got, st = form(ov, m)
            ck.assert_same_rows(got, want, seqs, m, "%s, %s" % (ctx, fname))
            assert st["kmer"] == min(max(m, 1), 64 // st["bits_per_base"]), (ctx, fname, st["kmer"])
            bits.add(st["bits_per_base"])
    finally:
        ov.close()
    assert len(bits) == 1, (ctx, bits)
    return bits.pop()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_small_goldens_under_the_maps(name, monkeypatch):
    monkeypatch.setenv("PHASM_HOST_CHUNKS", "3")
    f = MAPS[name]
    n8 = 0
    cases = gu.all_small_cases() + gu.repeats_cases()
    for case, seqs, m, want in cases:
        mapped = [f(s) for s in seqs]
        bits = check_forms(mapped, m, want, "%s %s" % (name, case),
                           FORMS if name == "swapcase" else {"whole": whole})
        n8 += bits == 8
        assert bits == expected_bits(mapped), case
    if name == "swapcase":
        assert n8 >= 250, n8           # (reads of 17 bases and more cannot hold their lower case as exception records)


@pytest.mark.parametrize("index", ["narrow", "wide"])
def test_small_goldens_soft_masked_both_index_flavours(index, monkeypatch):
    """The same small goldens, soft-masked, with the index flavour forced (the wide one where min_length >= 2W - 1 = 15 at
    8 bits, 63 at 2 bits)."""
    monkeypatch.setenv("PHASM_INDEX", index)
    n_wide8 = 0
    for case, seqs, m, want in gu.all_small_cases() + gu.repeats_cases():
        ov = handle([s.swapcase() for s in seqs])
        got, st = whole(ov, m)
        ov.close()
        ck.assert_same_rows(got, want, seqs, m, "%s, index %s" % (case, index))
        W = 64 // st["bits_per_base"]
        assert st["wide_index"] == (index == "wide" and max(m, 1) >= 2 * W - 1), (case, st["wide_index"])
        n_wide8 += st["wide_index"] == 1 and st["bits_per_base"] == 8
    assert (n_wide8 >= 4) == (index == "wide")   # (four small read sets go 8-bit with min_length >= 15)


@pytest.mark.parametrize("index", ["narrow", "wide"])
@pytest.mark.parametrize("ladder", gu.LADDER_NAMES)
def test_ladder_goldens_soft_masked(ladder, index, monkeypatch):
    """Every ladder golden, up to config 1 at full size, fully soft-masked: 8 bits per base in every form, both index
    flavours (narrow is also what these read sets get by default)."""
    monkeypatch.setenv("PHASM_INDEX", index)
    monkeypatch.setenv("PHASM_HOST_CHUNKS", "3")
    _, seqs, m, want = gu.ladder_case(ladder)
    mapped = [s.swapcase() for s in seqs]
    ov = handle(mapped)
    try:
        for fname, form in dict(FORMS, **{"candidates + expand": cands_expanded}).items():
            got, st = form(ov, m)
            ck.assert_same_rows(got, want, None, m, "%s soft-masked, index %s, %s" % (ladder, index, fname))
            assert st["bits_per_base"] == 8 and st["kmer"] == 8 and st["paired"] == 0, (fname, st)
            assert st["wide_index"] == (index == "wide"), (fname, st["wide_index"])
    finally:
        ov.close()


@pytest.mark.parametrize("ladder", ["ladder_varlen", "cfg3_1k"])
def test_ladder_goldens_under_the_code_rotation(ladder, monkeypatch):
    monkeypatch.setenv("PHASM_HOST_CHUNKS", "3")
    _, seqs, m, want = gu.ladder_case(ladder)
    ov = handle([s.translate(ROTATE) for s in seqs])
    try:
        for fname, form in FORMS.items():
            got, st = form(ov, m)
            ck.assert_same_rows(got, want, None, m, "%s rotated, %s" % (ladder, fname))
            assert st["bits_per_base"] == 2 and st["paired"] == 1, (fname, st)
    finally:
        ov.close()


def test_sliced_wide_index_at_8_bits(monkeypatch):
    """The multi-GPU index (tests/test_gpu_parity.py test_sliced_wide_index_equals_the_whole_index) on a soft-masked ladder."""
    import torch
    monkeypatch.setenv("PHASM_INDEX", "wide")
    _, seqs, m, want = gu.ladder_case("ladder_varlen")
    ov = handle([s.swapcase() for s in seqs])
    n_slices = 3
    try:
        built = [ov.index_slice_build(m, k, n_slices) for k in range(n_slices)]
        assert all(w for w, _, _ in built) and len({b for _, b, _ in built}) == 1
        bits, cap = built[0][1], max(e for _, _, e in built)
        chunk = ov.index_chunk_bytes(bits, cap)
        buf = torch.empty(n_slices * chunk, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for k in range(n_slices):
            assert ov.index_slice_build(m, k, n_slices) == built[k]
            ov.index_slice_export(buf.data_ptr() + k * chunk, cap)
        parts = [ov.overlaps_shard_indexed_array(m, k, n_slices, buf.data_ptr(), n_slices, bits, cap) for k in range(n_slices)]
        st = ov.stats()
        assert st["bits_per_base"] == 8 and st["wide_index"] == 1
        ck.assert_same_rows(_sorted(np.concatenate(parts)), want, None, m, "sliced wide index, 8 bits")
        got, st = whole(ov, m)
        ck.assert_same_rows(got, want, None, m, "whole index after the slices")
    finally:
        ov.close()


def _soft_masked_read_set(rng, trial):
    """A read set at byte mode's own edges: lengths around W = 8 and the 512-base tile, lower-case and N runs at the ends
    of reads over a 4-letter genome, tandem repeats, duplicates, both strands or one."""
    glen = int(rng.integers(300, 6000))
    if rng.random() < 0.3:
        unit = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=int(rng.integers(1, 12))))
        g = bytearray((unit * (glen // len(unit) + 1))[:glen])
        for pos in rng.integers(0, glen, size=glen // 50):
            g[pos] = b"ACGT"[rng.integers(4)]
        genome = bytes(g)
    else:
        genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=glen))
    # soft-masked stretches of the genome (shared by every read that covers them), N runs too
    g = bytearray(genome)
    for _ in range(int(rng.integers(0, 6))):
        a = int(rng.integers(0, glen))
        b = min(glen, a + int(rng.integers(1, 400)))
        g[a:b] = bytes(g[a:b]).lower() if rng.random() < 0.8 else b"N" * (b - a)
    genome = bytes(g)
    special = [1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025]
    reads = []
    for _ in range(int(rng.integers(4, 60))):
        ln = min(glen, int(rng.choice(special)) if rng.random() < 0.4 else int(rng.integers(1, 2500)))
        st = int(rng.integers(0, glen - ln + 1))
        r = bytearray(genome[st:st + ln])
        if ln and rng.random() < 0.5:    # a soft-masked or N run at one end of the read itself
            k = int(rng.integers(1, min(ln, 40) + 1))
            run = bytes(r[:k]).lower() if rng.random() < 0.7 else b"N" * k
            if rng.random() < 0.5:
                r[:k] = run
            else:
                r[ln - k:] = run[:k]
        r = bytes(r)
        if rng.random() < 0.5:
            r = revcomp(r)
        reads.append(r)
        if rng.random() < 0.1:
            reads.append(r)
    # at least one dense read: byte mode for the whole set
    reads.append(genome[:min(glen, 200)].lower())
    if rng.random() < 0.6:
        return [x for r in reads for x in (r, revcomp(r))]
    return reads


@pytest.mark.parametrize("index", ["narrow", "wide"])
def test_seeded_fuzz_at_8_bits_against_oracle(index, monkeypatch):
    """The 8-bit counterpart of test_seeded_fuzz_against_oracle: min_length below, at and above W = 8 (kmer == m selects
    the partial-K-mer probe), around the wide index's 2W - 1 = 15, whole set and 3 shards."""
    monkeypatch.setenv("PHASM_INDEX", index)
    rng = np.random.default_rng(int(os.environ.get("PHASM_FUZZ_SEED", "2024")) + 8)
    n_short_k = 0
    for trial in range(int(os.environ.get("PHASM_FUZZ_TRIALS", "30"))):
        seqs = _soft_masked_read_set(rng, trial)
        m = int(rng.choice([1, 2, 7, 8, 9, 14, 15, 16, 39, 40, 100]))
        want = ck.oracle_overlaps(seqs, m)
        ov = handle(seqs)
        try:
            got, st = whole(ov, m)
            ctx = "trial %d m %d reads %d wide %d" % (trial, m, len(seqs), st["wide_index"])
            assert st["bits_per_base"] == 8 and st["kmer"] == min(m, 8), ctx
            assert st["wide_index"] == (index == "wide" and m >= 15), ctx
            n_short_k += m < 8
            ck.assert_same_rows(got, want, seqs, m, ctx)
            got3, _ = sharded(ov, m)
            ck.assert_same_rows(got3, want, seqs, m, ctx + ", 3 shards")
        finally:
            ov.close()
    assert n_short_k > 0 or int(os.environ.get("PHASM_FUZZ_TRIALS", "30")) < 10


def test_long_soft_masked_reads_around_the_lds_staging_limit():
    """k_verify_a stages a's words in LDS when ceil(len_a / W) + 3 <= lds_words, lds_words being the even part of
    min(ceil(max_len / W) + 3, 8192 - 1100) = 7092 words once some read is that long (c_api.hip run_overlaps, verify
    launch).  At 8 bits per base (W = 8) that is 7089 words: reads of up to 56 712 bases compare from LDS, longer ones from
    global memory.  Reads just below, at and above the cut, and one of 150 kb, both strands, lower case."""
    rng = np.random.default_rng(88)
    genome = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=400_000)].tobytes()
    cut = 7089 * 8
    spans = [(0, cut - 8), (40_000, 40_000 + cut), (90_000, 90_000 + cut + 1), (95_000, 95_000 + cut + 9),
             (140_000, 290_000), (280_000, 281_500), (289_000, 300_000), (0, 20_000)]
    seqs = []
    for a, b in spans:
        r = genome[a:b]
        seqs += [r, revcomp(r)]
    want = ck.oracle_overlaps(seqs, 1000)
    assert len(want) >= 8
    ov = handle(seqs)
    try:
        for fname, form in FORMS.items():
            got, st = form(ov, 1000)
            assert st["bits_per_base"] == 8, fname
            ck.assert_same_rows(got, want, seqs, 1000, "long 8-bit reads, %s" % fname)
    finally:
        ov.close()


@pytest.mark.parametrize("first", ["resident", "streamed"])
def test_switch_to_8_bits_on_a_live_handle(first, monkeypatch):
    """A 2-bit handle with exception records makes a call (resident, or the streamed step), then a dense soft-masked read
    pair arrives: the store is re-encoded at 8 bits (materialize: codes, then the records on top), the next calls must
    not stream (the streamed step serves 2-bit reads only) and must not reuse the 2-bit index."""
    monkeypatch.setenv("PHASM_STREAM", "1" if first == "streamed" else "0")
    monkeypatch.setenv("PHASM_STREAM_CUTS", "300,700")
    rng = np.random.default_rng(404)
    genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=20_000))
    seqs = []
    for _ in range(150):
        ln = int(rng.integers(200, 3000))
        st0 = int(rng.integers(0, len(genome) - ln))
        r = bytearray(genome[st0:st0 + ln])
        for i in {0, 31, 32, ln - 1} if rng.random() < 0.5 else {int(rng.integers(0, ln))}:
            r[i] = b"NacR"[int(rng.integers(4))]
        r = bytes(r)
        seqs += [r, revcomp(r).translate(bytes.maketrans(b"RY", b"YR"))]
    m = 40
    ov = handle(seqs)
    try:
        got, st = (to_host if first == "streamed" else whole)(ov, m)
        assert st["bits_per_base"] == 2 and st["paired"] == 1 and st["streamed"] == (first == "streamed"), st
        ck.assert_same_rows(got, ck.oracle_overlaps(seqs, m), seqs, m, "2 bits with exception records")
        dense = genome[5000:7000].lower()
        for x in (dense, revcomp(dense)):
            ov.add_sequence("r%d" % len(seqs), x)
            seqs.append(x)
        want = ck.oracle_overlaps(seqs, m)
        got, st = to_host(ov, m)
        assert st["bits_per_base"] == 8 and st["streamed"] == 0 and st["index_reused"] == 0, st
        ck.assert_same_rows(got, want, seqs, m, "after the switch to 8 bits, to_host")
        got, st = whole(ov, m)
        assert st["bits_per_base"] == 8
        ck.assert_same_rows(got, want, seqs, m, "after the switch to 8 bits, whole")
    finally:
        ov.close()


def test_cli_on_a_soft_masked_fasta(tmp_path):
    """The overlap command on the lower-cased FASTA of tests/test_gpu_e2e.py's case against the upper-case file (native
    ingest takes its record-by-record path there; the reverse complement of lower case goes through the IUPAC table).
    Header and S lines equal line for line; E lines equal byte for byte as a multiset.  Their order is the device's emission
    order (phasm_amd/cli.py), which the two paths -- strand-paired 2-bit reads, unpaired 8-bit reads -- give differently."""
    from phasm_amd import cli, synth
    _, _, m, _ = gu.ladder_case("ladder_small")
    cfg = synth.SynthConfig(n_reads=80, read_len=2000, genome_len=10_000, ploidy=2, snp=0.005, seed=11)
    reads = synth.generate_reads(cfg)
    fa, fa_lc = tmp_path / "reads.fasta", tmp_path / "reads_lc.fasta"
    synth.write_fasta(str(fa), reads, width=70)
    synth.write_fasta(str(fa_lc), [(n, s.lower()) for n, s in reads], width=70)
    out, out_lc = tmp_path / "out.gfa", tmp_path / "out_lc.gfa"
    assert cli.main(["overlap", str(fa), "-l", str(m), "-o", str(out)]) == 0
    assert cli.main(["overlap", str(fa_lc), "-l", str(m), "-o", str(out_lc)]) == 0
    lines_up, lines_lc = out.read_text().splitlines(), out_lc.read_text().splitlines()
    e_up = [l for l in lines_up if l.startswith("E\t")]
    e_lc = [l for l in lines_lc if l.startswith("E\t")]
    assert len(e_up) > 0
    assert lines_lc[:len(lines_lc) - len(e_lc)] == lines_up[:len(lines_up) - len(e_up)]   # H and S lines, in order
    assert sorted(e_lc) == sorted(e_up)
