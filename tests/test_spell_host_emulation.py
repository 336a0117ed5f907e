"""The kernels of po_spell compiled for the HOST (tools/spell_host_emu.cpp: threads one after another) against the goldens, with
AddressSanitizer + UBSan: the search for a chunk's piece, the walk over short and empty pieces, the words a fetch loads (the
emulator's store has no byte behind a read's guard word to spare), the letters, the upper-casing in the word, the bound of the
patch, launched as c_api.hip launches them, checked without a GPU; and against plain Python slicing on the sweep and the odd
bytes of tests/spell_store_utils.py.  The program is a stand-alone executable run as a
subprocess on a case file; every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import pytest

import emu_utils
import spell_store_utils as ssu
import spell_utils as su
from phasm_amd import spelling

emu = emu_utils.emu_fixture("spell")


def run_emu(emu, tmp_path, reads, seq_off, piece_read, piece_take, bits=0, first_byte=0, n_out=0, offsets=None):
    text = ["%d %d %d %d %d %d %d" % (bits, len(reads), len(piece_read), len(seq_off) - 1, first_byte, n_out, offsets is not None)]
    text += [s.hex() or "-" for s in reads]
    text += ["%d %d" % (r, t) for r, t in zip(piece_read, piece_take)]
    text.append(" ".join(str(int(x)) for x in seq_off))
    if offsets is not None:
        text.append(" ".join(str(int(x)) for x in offsets))
    path = tmp_path / "case.txt"
    path.write_text("\n".join(text) + "\n")
    out = subprocess.run([emu, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    head, soff, blob = out.stdout.split("\n")[:3]
    return [int(x) for x in head.split()], [int(x) for x in soff.split()], bytes.fromhex(blob)


@pytest.mark.parametrize("which", ["main", "wide"])
def test_host_compiled_kernels_equal_the_golden(emu, tmp_path, which):
    """Every golden call of a read set, and all of them as ONE call."""
    reads = [s for _, s in su.oriented(su.records(which))]
    reads_of = spelling.ReadMap.of(su.host_speller(which))
    everything, want_all = [], []
    for case in su.good_cases(which):
        pieces = su.pieces_of(case, reads_of)
        want = su.expected_bytes(case)
        seq_off, pr, pt = su.call_arrays(pieces)
        head, soff, blob = run_emu(emu, tmp_path, reads, seq_off, pr, pt)
        assert head[0] == (8 if which == "wide" else 2) and head[1] == len(b"".join(want)), case["name"]
        assert [blob[soff[i]:soff[i + 1]] for i in range(len(want))] == want, case["name"]
        everything += pieces
        want_all += want
    seq_off, pr, pt = su.call_arrays(everything)
    head, soff, blob = run_emu(emu, tmp_path, reads, seq_off, pr, pt)
    assert [blob[soff[i]:soff[i + 1]] for i in range(len(want_all))] == want_all
    if which == "main":
        hs = su.host_speller(which)
        hs.spell(seq_off, pr, pt)
        assert head[2] == hs.spell_stats()["n_patched"] > 0   # the exception records inside the pieces, counted on both sides


def test_the_main_read_set_as_bytes(emu, tmp_path):
    """The 8-bit branch on the reads of the 2-bit goldens (a handle widens for ALL its reads)."""
    reads = [s for _, s in su.oriented(su.records("main"))]
    reads_of = spelling.ReadMap.of(su.host_speller("main"))
    for name in ("exceptions_X70-", "ones_and_zeros", "every_residue", "merged_cut", "takes_L200+"):
        case = next(c for c in su.good_cases("main") if c["name"] == name)
        seq_off, pr, pt = su.call_arrays(su.pieces_of(case, reads_of))
        head, soff, blob = run_emu(emu, tmp_path, reads, seq_off, pr, pt, bits=8)
        assert head[0] == 8 and blob == b"".join(su.expected_bytes(case)), name


@pytest.mark.parametrize("bits", [2, 8])
def test_offsets_just_below_and_beyond_2_to_the_32(emu, tmp_path, bits):
    """A synthetic output longer than one call may make: the piece offsets are GIVEN, the kernels write a window of 64 bytes
    that straddles 2^32, so the search, the walk and the patch run their 64-bit arithmetic."""
    sp = su.host_speller("main")
    reads = [s for _, s in su.oriented(su.records("main"))]
    x70, s9, big = sp.ids().index("X70+"), sp.ids().index("s9-"), sp.ids().index("L2049+")
    pieces = [(big, 2049), (x70, 34), (s9, 0), (s9, 1), (x70, 70), (s9, 10), (big, 500)]
    first = 2**32 - 48                              # the window: [2^32 - 48, 2^32 + 16)
    start = first - 2049 + 7                        # the first piece ends 7 bytes into the window
    off = [start]
    for _, t in pieces:
        off.append(off[-1] + t)
    want = b"".join(sp.spell([0, len(pieces)], [p[0] for p in pieces], [p[1] for p in pieces]))
    head, soff, blob = run_emu(emu, tmp_path, reads, [0, len(pieces)], [p[0] for p in pieces], [p[1] for p in pieces], bits=bits,
                               first_byte=first, n_out=64, offsets=off)
    assert off[1] < 2**32 < off[5] and soff == [off[0], off[-1]]
    assert blob == want[first - start:first - start + 64]


# ---- against plain slicing: the sweep and the odd bytes (tests/spell_store_utils.py) -----------------------------------------

def emu_spelled(emu, tmp_path, reads, call, bits):
    seq_off, pr, pt = call
    head, soff, blob = run_emu(emu, tmp_path, reads, seq_off, pr, pt, bits=bits)
    return head, [blob[soff[i]:soff[i + 1]] for i in range(len(soff) - 1)]


@pytest.mark.parametrize("bits", [2, 8])
def test_the_sweep_on_host_compiled_kernels(emu, tmp_path, bits):
    """Output-offset residue x read x take around the 32-base and 8-byte word edges, in both encodings (the whole sweep in
    one run: a fifth of a second under the sanitizers)."""
    reads = ssu.edge_reads()
    call = ssu.sweep_call(reads)
    want = ssu.plain_spell(reads, *call)
    head, got = emu_spelled(emu, tmp_path, reads, call, bits)
    assert (len(want), len(call[1]), head[1]) == ssu.SWEEP_SIZE
    assert head == [bits, sum(map(len, want)), ssu.count_patched(reads, call[1], call[2], bits)]
    assert ssu.first_difference(got, want) is None


@pytest.mark.parametrize("which", [0, 1], ids=["2-bit", "8-bit"])
def test_the_bytes_next_to_a_z_on_host_compiled_kernels(emu, tmp_path, which):
    """@ [ ` { 0x80 0xE1 0xFA 0xFF and a z A Z N n as exception records of a 2-bit store (k_spell_patch, spell_upper) and in
    the words of an 8-bit one (spell_upper8), at the width the library itself would choose for the set."""
    reads = ssu.odd_bytes_reads()[which]
    bits = (2, 8)[which]
    for call in (ssu.whole_reads_call(reads), ssu.random_call(reads, 23)):
        head, got = emu_spelled(emu, tmp_path, reads, call, 0)
        assert head[0] == bits and head[2] == ssu.count_patched(reads, call[1], call[2], bits)
        assert ssu.first_difference(got, ssu.plain_spell(reads, *call)) is None
