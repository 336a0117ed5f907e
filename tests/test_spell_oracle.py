"""The host side of spelling against what the reference's own sequence_for_path, node_path_edges and get_sequence gave
(tests/golden/spell_cases.npz, made by tests/golden/make_spell_golden.py): the piece builder of phasm_amd/spelling.py against
the recorded pieces and errors, HostSpeller over the pieces against the recorded bytes, linear_order against the recorded
orders.  Three broken spellers show that the cases notice what they are there for.  No GPU; every comparison is exact."""
import numpy as np
import pytest

import spell_utils as su
from phasm_amd import spelling

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
