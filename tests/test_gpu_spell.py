"""po_spell on the device against tests/golden/spell_cases.npz (the reference's own sequence_for_path, node_path_edges and
get_sequence): every golden call through ExactOverlapper.spell with byte equality, on a 2-bit handle and on one widened to 8
bits per base, twice, after a larger and after a smaller call on the same handle; one call past a capped grid against
HostSpeller; the capacity refusal and the rejections of the C ABI; `spell-contigs` end to end."""
import numpy as np
import pytest

import spell_utils as su
from phasm_amd import cli, spelling
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    out = {w: su.add_reads(ExactOverlapper(), w) for w in ("main", "wide")}
    yield out
    for ov in out.values():
        ov.close()


@pytest.mark.parametrize("which", ["main", "wide"])
def test_device_equals_the_golden(handles, which):
    ov = handles[which]
    reads_of = spelling.ReadMap.of(ov)
    calls = [(c["name"], su.call_arrays(su.pieces_of(c, reads_of)), su.expected_bytes(c)) for c in su.good_cases(which)]
    everything = su.call_arrays([ps for c in su.good_cases(which) for ps in su.pieces_of(c, reads_of)])
    want_all = [b for _, _, want in calls for b in want]
    for name, arrays, want in calls:
        assert ov.spell(*arrays) == want, name
        st = ov.spell_stats()
        assert (st["n_seqs"], st["n_pieces"], st["n_bytes"]) == (len(want), len(arrays[1]), sum(map(len, want))), name
        assert ov.spell(*arrays) == want, name + " (again)"
    # a larger call, then the smaller ones again in workspaces and a spare output buffer that have held more
    assert ov.spell(*everything) == want_all
    n_patched = ov.spell_stats()["n_patched"]
    assert (n_patched > 0) == (which == "main")       # (a widened handle has no exception records)
    for name, arrays, want in reversed(calls):
        assert ov.spell(*arrays) == want, name + " (after the large call)"
    assert ov.spell(*everything) == want_all
    assert ov.spell([0], [], []) == [] and ov.spell([0, 0, 0], [], []) == [b"", b""]


def test_a_call_past_one_capped_grid():
    reads, seq_off, piece_read, piece_take = su.big_call()
    ov = ExactOverlapper()
    for name, seq in reads:
        ov.add_sequence(name, seq)
    got = ov.spell(seq_off, piece_read, piece_take)
    st = ov.spell_stats()
    ov.close()
    want = spelling.HostSpeller([s for _, s in reads]).spell(seq_off, piece_read, piece_take)
    assert st["n_pieces"] == 600_000 and st["n_bytes"] > 9_000_000 and st["n_bytes"] // 16 > 524_288 and st["n_patched"] > 0
    assert len(got) == len(want) == 1000 and got == want


def test_the_capacity_refusal_leaves_the_handle_usable(handles):
    ov = handles["main"]
    long_read = ov.ids().index("L2049+")
    k = (2**32 - 16) // 2049 + 1
    with pytest.raises(OverflowError, match="2\\^32 - 16"):
        ov.spell([0, k], np.full(k, long_read, dtype=np.uint32), np.full(k, 2049, dtype=np.uint32))
    case = next(c for c in su.good_cases("main") if c["name"] == "merged_nodes")
    assert ov.spell(*su.call_arrays(su.pieces_of(case, spelling.ReadMap.of(ov)))) == su.expected_bytes(case)


def test_rejections(handles):
    ov = handles["main"]
    n, first_len = len(ov), int(ov.lengths()[0])
    with pytest.raises(ValueError, match="names read"):
        ov.spell([0, 1], [n], [0])
    with pytest.raises(ValueError, match="takes"):
        ov.spell([0, 1], [0], [first_len + 1])
    with pytest.raises(ValueError, match="seq_off"):
        ov.spell([0, 2], [0], [1])
    with pytest.raises(ValueError, match="seq_off"):
        ov.spell([1, 1], [0], [1])
    with pytest.raises(ValueError, match="ascending"):
        ov.spell([0, 2, 1, 2], [0, 0], [1, 1])
    assert ov.spell([0, 1], [0], [first_len]) == [su.oriented(su.records("main"))[0][1].upper()]
    segs = ExactOverlapper()
    segs.add_segment("a", 100)
    with pytest.raises(ValueError, match="po_add_segment"):
        segs.spell([0, 1], [0], [10])
    segs.close()


def test_spell_contigs_end_to_end(tmp_path):
    fasta = tmp_path / "reads.fasta"
    fasta.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in su.records("main")))
    names = ("ones_and_zeros", "single_merged_node", "every_residue")
    want = b""
    paths = []
    for name in names:
        case = next(c for c in su.good_cases("main") if c["name"] == name)
        p = tmp_path / ("%s.contig.gfa" % name)
        p.write_text(case["gfa"])
        paths.append(str(p))
        want += b">" + name.encode() + b".contig\n" + su.expected_bytes(case)[0] + b"\n"
    out = tmp_path / "contigs.fasta"
    assert cli.main(["spell-contigs", str(fasta), *paths, "-o", str(out)]) == 0
    assert out.read_bytes() == want
    # a graph that is no simple path is an error that names the file
    fork = tmp_path / "fork.gfa"
    fork.write_text(next(o for o in su.load_golden()["orders"] if o["name"] == "fork")["gfa"])
    with pytest.raises(SystemExit, match="fork.gfa"):
        cli.main(["spell-contigs", str(fasta), paths[0], str(fork), "-o", str(tmp_path / "none.fasta")])
