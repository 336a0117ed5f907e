"""The host side of spelling against what the reference's own sequence_for_path, node_path_edges and get_sequence gave
(tests/golden/spell_cases.npz, made by tests/golden/make_spell_golden.py): the piece builder of phasm_amd/spelling.py against
the recorded pieces and errors, HostSpeller over the pieces against the recorded bytes, linear_order against the recorded
orders.  Three broken spellers show that the cases notice what they are there for.  Then HostSpeller against plain Python
slicing on the calls of the store tests (tests/spell_store_utils.py: the sweep, the whole reads, the odd bytes), and three
models of kernel mistakes that those calls must notice.  No GPU; every comparison is exact."""
import numpy as np
import pytest

import spell_store_utils as ssu
import spell_utils as su
from phasm_amd import spelling
from phasm_amd.io.fasta import reverse_complement

ALL = su.cases()
GOOD = [c for c in ALL if not c["error"]]
BAD = [c for c in ALL if c["error"]]
ORDERS = su.load_golden()["orders"]


@pytest.fixture(scope="module")
def spellers():
    return {w: su.host_speller(w) for w in ("main", "wide")}


@pytest.fixture(scope="module")
def maps(spellers):
    return {w: spelling.ReadMap.of(s) for w, s in spellers.items()}


def test_the_golden_holds_the_cases_the_kernels_can_go_wrong_at():
    takes = {t for c in GOOD for ps in c["pieces"] for _, t in ps}
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 199, 200, 2048, 2049} <= takes
    ones = next(c for c in GOOD if c["name"] == "ones_and_zeros")["pieces"][0]
    assert len(ones) >= 40
    off = np.cumsum([0] + [t for _, t in next(c for c in GOOD if c["name"] == "every_residue")["pieces"][0]])
    assert {int(o) % 16 for o in off[:-1]} == set(range(16))
    assert any(len(b) == 0 for c in GOOD for b in c["bytes"]) and any(c["paths"] == [] for c in GOOD)
    assert {c["reads"] for c in GOOD} == {"main", "wide"} and len(BAD) >= 4


@pytest.mark.parametrize("name", [c["name"] for c in GOOD])
def test_pieces_equal_the_recorded_ones(maps, name):
    case = next(c for c in GOOD if c["name"] == name)
    got = su.pieces_of(case, maps[case["reads"]])
    assert [[list(p) for p in ps] for ps in got] == case["pieces"]


@pytest.mark.parametrize("name", [c["name"] for c in BAD])
def test_what_the_reference_refuses_is_refused(maps, name):
    case = next(c for c in BAD if c["name"] == name)
    with pytest.raises(ValueError):
        su.pieces_of(case, maps[case["reads"]])


def spelled(speller, case, reads_of):
    return speller.spell(*su.call_arrays(su.pieces_of(case, reads_of)))


@pytest.mark.parametrize("which", ["main", "wide"])
def test_host_speller_equals_the_reference(spellers, maps, which):
    for case in su.good_cases(which):
        assert spelled(spellers[which], case, maps[which]) == su.expected_bytes(case), case["name"]
    assert spellers[which].spell([0], [], []) == []
    st = spellers[which].spell_stats()
    assert st["n_seqs"] == 0 and st["n_bytes"] == 0


def test_spell_paths_is_one_call_over_many_paths(spellers):
    case = next(c for c in GOOD if c["name"] == "merged_nodes")
    gf = su.graph_of(case)
    keep = [i for i, last in enumerate(case["include_last"]) if last]
    got = spelling.spell_paths(spellers["main"], gf, [[su.node_id(gf, n) for n in case["paths"][i]] for i in keep], True)
    assert got == [su.expected_bytes(case)[i] for i in keep]
    assert spellers["main"].spell_stats()["n_seqs"] == len(keep)


def test_host_speller_refuses_what_the_library_refuses(spellers):
    sp = spellers["main"]
    n = len(sp)
    with pytest.raises(ValueError):
        sp.spell([0, 1], [n], [0])                 # a read the speller does not hold
    with pytest.raises(ValueError):
        sp.spell([0, 1], [0], [int(sp.lengths()[0]) + 1])   # a take longer than the read
    with pytest.raises(ValueError):
        sp.spell([0, 2], [0], [1])                 # seq_off does not end at n_pieces
    with pytest.raises(ValueError):
        sp.spell([0, 2, 1, 2], [0, 0], [1, 1])     # seq_off not ascending
    with pytest.raises(ValueError):
        sp.spell([0, 1], [0, 0], [1])              # two lengths
    long_read = sp.ids().index("L2049+")
    k = (2**32 - 16) // 2049 + 1
    with pytest.raises(OverflowError):
        sp.spell([0, k], np.full(k, long_read, dtype=np.uint32), np.full(k, 2049, dtype=np.uint32))


def test_slicing_cases():
    assert [spelling.slice_take(10, w) for w in (0, 3, 10, 11, -1, -10, -11)] == [0, 3, 10, 10, 9, 0, 0]
    assert spelling.truncate_pieces([(4, 3), (5, 0), (6, 5)], 4) == [(4, 3), (5, 0), (6, 1)]
    assert spelling.truncate_pieces([(4, 3), (6, 5)], -6) == [(4, 2), (6, 0)]


@pytest.mark.parametrize("name", [o["name"] for o in ORDERS])
def test_linear_order(name):
    o = next(x for x in ORDERS if x["name"] == name)
    gf = su.graph_of(o)
    if o["error"]:
        with pytest.raises(ValueError, match="not a simple path"):
            spelling.linear_order(gf)
    else:
        assert [gf.node_name(n) for n in spelling.linear_order(gf)] == o["order"]


# ---- three broken spellers, each noticed by the cases that are there for it ------------------------------------------------

def failing_cases(speller, reads_of, which="main"):
    bad = []
    for case in su.good_cases(which):
        if spelled(speller, case, reads_of) != su.expected_bytes(case):
            bad.append(case["name"])
    return bad


class UnboundedPatch(spelling.HostSpeller):
    def _records_end(self, start, take, length):   # every record of the read, not only those with pos < take
        return start + length


class NoUpperCase(spelling.HostSpeller):
    def _case(self, b):
        return b


def test_a_broken_speller_is_noticed(spellers, maps, monkeypatch):
    assert failing_cases(spellers["main"], maps["main"]) == []
    # exception records patched without the `pos < take` bound: they land in the bytes of the pieces behind
    bad = failing_cases(su.host_speller("main", UnboundedPatch), maps["main"])
    assert {"exceptions_X70+", "exceptions_X70-"} <= set(bad) and "takes_L200+" not in bad, bad
    # upper-casing left out
    bad = failing_cases(su.host_speller("main", NoUpperCase), maps["main"])
    assert {"exceptions_X70+", "exceptions_X70-", "no_acgt_at_all"} <= set(bad) and "takes_L200+" not in bad, bad
    # a prefix length of 0 taken as "0 bytes" instead of the whole read
    monkeypatch.setattr(spelling, "prefix_take", lambda prefix, n: n if prefix is None else spelling.slice_take(n, prefix))
    bad = failing_cases(spellers["main"], maps["main"])
    assert {"merged_cut", "merged_nodes", "single_merged_node"} <= set(bad) and "takes_L200+" not in bad, bad


# ---- HostSpeller against plain slicing, on the calls the device tests make (tests/spell_store_utils.py) ---------------------

@pytest.fixture(scope="module")
def edge_sweep():
    reads = ssu.edge_reads()
    call = ssu.sweep_call(reads)
    return reads, call, ssu.plain_spell(reads, *call)


def test_the_sweep_is_the_product_it_says(edge_sweep):
    reads, (seq_off, pr, pt), want = edge_sweep
    assert sorted(len(s) for s in reads[::2]) == list(ssu.EDGE_LENGTHS) and len(reads) == 56
    assert all(reads[2 * i + 1] == reverse_complement(reads[2 * i]) for i in range(28))
    assert (len(want), len(pr), sum(map(len, want))) == ssu.SWEEP_SIZE
    lens = [len(s) for s in reads]
    seen = {(int(pt[3 * s]), int(pr[3 * s + 1]), int(pt[3 * s + 1])) for s in range(len(want))}
    assert seen == {(o, r, t) for o in range(16) for r in range(56) for t in ssu.sweep_takes(lens[r])}
    assert ssu.sweep_takes(65) == list(range(66)) and ssu.sweep_takes(96) == [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96]
    # every third non-empty record holds the exception bytes at its ends and around the word edge
    with_exc = [s for s in reads[::2] if ssu.exception_positions(s)]
    assert len(with_exc) == 9 and all({0, len(s) - 1, min(32, len(s) - 1)} <= set(ssu.exception_positions(s)) for s in with_exc)
    assert ssu.expected_bits(reads) == 2 and ssu.expected_bits(reads + [ssu.dense_read()]) == 8


def test_host_speller_equals_plain_slicing(edge_sweep):
    reads, call, want = edge_sweep
    hs = spelling.HostSpeller(reads)
    assert ssu.first_difference(hs.spell(*call), want) is None
    assert hs.spell_stats()["n_patched"] == ssu.count_patched(reads, call[1], call[2], 2) > 0
    whole = ssu.whole_reads_call(reads)
    assert hs.spell(*whole) == ssu.plain_spell(reads, *whole) == [s.upper() for s in reads]
    for odd in ssu.odd_bytes_reads():
        hs = spelling.HostSpeller(odd)
        for call in (ssu.whole_reads_call(odd), ssu.random_call(odd, 5)):
            assert ssu.first_difference(hs.spell(*call), ssu.plain_spell(odd, *call)) is None


def test_the_odd_byte_sets_hold_what_they_are_there_for():
    a, b = ssu.odd_bytes_reads()
    assert ssu.expected_bits(a) == 2 and ssu.expected_bits(b) == 8 and b[:-1] == a and all(200 <= len(s) <= 300 for s in a)
    for c in ssu.ODD_BYTES:
        for pos in ssu.ODD_POSITIONS:
            assert any(s[pos] == c for s in a), (c, pos)
        assert {i % 8 for i, x in enumerate(b[-1]) if x == c} == set(range(8)), c
    assert all(len(ssu.exception_positions(s)) < len(s) // 64 + 16 for s in a)
    # (upper-casing moves a-z and nothing else, in the reference of these tests too)
    assert bytes(range(256)).upper() == bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))


# ---- three models of kernel mistakes, each noticed by the sweep or the odd bytes ---------------------------------------------

class UpperOnSevenBits(spelling.HostSpeller):
    """spell_upper / spell_upper8 without their test of bit 7: 0xE1 .. 0xFA lose 32 like a .. z."""
    def _case(self, b):
        table = np.arange(256, dtype=np.uint8)
        table[[c for c in range(256) if 97 <= (c & 0x7F) <= 122]] -= 32
        return table[b]


class PatchStopsOneEarly(spelling.HostSpeller):
    """k_spell_patch with the bound `pos < take - 1`: the record at the last byte of a piece is dropped."""
    def _records_end(self, start, take, length):
        return start + np.maximum(take - 1, 0)


class LateSecondWord(spelling.HostSpeller):
    """spell_fetch<2> that loads the second word only when (skip & 31) + n > 33: a fetch whose last base is the first of the
    next word gets code 0 there, `A`, unless an exception record is patched over it afterwards.  The fetches are those of
    k_spell_decode: a piece cut at the 16-byte chunks of the output."""
    def spell(self, seq_off, piece_read, piece_take):
        out = super().spell(seq_off, piece_read, piece_take)
        blob, off = bytearray(b"".join(out)), 0
        for r, take in zip(np.asarray(piece_read).tolist(), np.asarray(piece_take).tolist()):
            pos = off
            while pos < off + take:
                end = min(off + take, (pos // 16 + 1) * 16)
                if ((pos - off) & 31) + (end - pos) == 33 and self._seqs[r][end - 1 - off] in b"ACGT":
                    blob[end - 1] = ord("A")
                pos = end
            off += take
        cuts = np.cumsum([0] + [len(b) for b in out]).tolist()
        return [bytes(blob[cuts[s]:cuts[s + 1]]) for s in range(len(out))]


def test_three_models_of_kernel_mistakes_are_noticed(edge_sweep):
    reads, call, want = edge_sweep
    odd_a, odd_b = ssu.odd_bytes_reads()

    def differs(cls, rs, c):
        return ssu.first_difference(cls(rs).spell(*c), ssu.plain_spell(rs, *c)) is not None
    for cls in (spelling.HostSpeller, UpperOnSevenBits, PatchStopsOneEarly, LateSecondWord):
        broken = cls is not spelling.HostSpeller
        on_sweep, on_odd = differs(cls, reads, call), differs(cls, odd_a, ssu.whole_reads_call(odd_a))
        assert (on_sweep or on_odd) == broken, cls.__name__
        if cls is UpperOnSevenBits:
            assert on_odd and not on_sweep            # (the edge reads hold no byte >= 0x80: only the odd bytes see it)
        if cls in (PatchStopsOneEarly, LateSecondWord):
            assert on_sweep, cls.__name__
