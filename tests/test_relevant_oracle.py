"""po_phase_index / po_phase_relevant without a GPU: the dict-of-dicts ``definition`` and the numpy ``HostIndex`` against the
goldens recorded from the reference's own methods (index entries with their sequence numbers included), the Python layer
(``relevant_reads``, ``bubble_from_relevant``) down to the kept list of ``branch``, and ``device_phaser`` with an index on a
stand-in class.  All results of the gather are integers: exact equality."""
import os
import sys

import numpy as np
import pytest

import phase_utils as pu
import relevant_utils as ru
from phasm_amd import phasing

CASES = ru.load_golden()["cases"]
NAMES = [c["name"] for c in CASES]


def test_the_cases_are_the_specs():
    assert NAMES == list(ru.SPECS)
    for c in CASES:
        spec = ru.SPECS[c["name"]]()
        assert c["rows_flat"] == spec["rows_flat"] and c["lengths"] == spec["lengths"] and c["queries"] == spec["queries"]
        assert (2 * c["n_seg"]) % 64 != 0


@pytest.mark.parametrize("name", NAMES)
def test_definition_equals_the_golden(name):
    case = next(c for c in CASES if c["name"] == name)
    off, entries = ru.index_definition(case)
    want_off, want = ru.golden_index(case)
    assert off == list(want_off) and entries == [tuple(w) for w in want]
    m = ru.mapping(case)
    for i, (q, ref) in enumerate(zip(case["queries"], case["results"])):
        ru.same_result(ru.definition(case, q, m), ref, "%s q%d" % (name, i))


@pytest.mark.parametrize("name", NAMES)
def test_host_index_equals_the_golden(name):
    case = next(c for c in CASES if c["name"] == name)
    host = phasing.HostIndex(ru.lengths_of(case))
    index = host.phase_index(ru.rows_array(ru.rows_of(case)))          # (structured rows, as the device takes them)
    ru.same_index(*host.phase_index_entries(index), *ru.golden_index(case))
    for i, (q, ref) in enumerate(zip(case["queries"], case["results"])):
        ru.same_result(ru.query_source(host, index, q), ref, "%s q%d" % (name, i))


def test_the_two_consequences_of_the_write_order():
    host = phasing.HostIndex([10] * 6)
    _, e = host.phase_index_entries(host.phase_index(np.array([[0, 2, 1, 2, 3, 4], [2, 0, 5, 6, 7, 8], [4, 4, 1, 2, 8, 9]])))
    assert e.tolist() == [(2, 7, 8, 3), (0, 5, 6, 2), (4, 8, 9, 5)]   # (0, 2) and (2, 0) from the later row; (4, 4) = (bstart, bend)


@pytest.mark.parametrize("pc", ru.chain_cases(), ids=lambda pc: pc["name"])
def test_the_chain_gives_the_kept_list_of_pack_bubble(pc):
    x = ru.phase_case_as_rows(pc)
    host, scorer = phasing.HostIndex(np.repeat(x["lengths"], 2)), phasing.HostScorer()
    index = host.phase_index(x["rows"])
    rel = phasing.relevant_reads(host, index, x["cur_graph"], [], x["prev_aligning"], x["preds"], False, pc["min_span"])
    assert not rel.fell_back and rel.rel_reads.tolist() == x["prev_aligning"] and rel.overlap_max.tolist() == list(pc["overlap_max"])
    bubble = phasing.bubble_from_relevant(rel, pc["k"], x["paths"], x["read_sets"])
    got = pu.result_of(scorer, ru.chained_case(pc, bubble))
    pu.check_result(got, pc["ref"], pc)
    # pack_bubble on the same objects (the global ids): another numbering, the same kept list
    relevant = {int(r): (rel.alignments_of(j), int(rel.overlap_max[j])) for j, r in enumerate(rel.rel_reads)}
    packed = phasing.pack_bubble([("in", *p, "out") for p in x["paths"]], x["read_sets"], relevant, expand=lambda node: (node,))
    want = pu.result_of(scorer, ru.chained_case(pc, packed))
    assert got["kept_cand"] == want["kept_cand"] and got["kept_ext"] == want["kept_ext"] and got["surv"] == want["surv"]
    assert all(pu.same_rl(g, w, pc["k"], pc["R"]) for g, w in zip(got["kept_rl"], want["kept_rl"]))


def test_bubble_from_relevant_drops_ids_outside_b_reads():
    case = next(c for c in CASES if c["name"] == "bubble")
    host = phasing.HostIndex(ru.lengths_of(case))
    q = case["queries"][2]
    rel = host.phase_relevant(host.phase_index(ru.rows_of(case)), q["cur_graph"], q["prev_graph"], q["prev_aligning"], q["preds"], 0, 2)
    b = phasing.bubble_from_relevant(rel, 2, [[20, 22, 30], [24, 24, 58]], [[[10, 34], []], [[12], [20, 26]]])
    assert b.b_reads == [10, 12, 20, 22, 24, 26] and (b.n_paths, b.n_cands, b.n_reads, b.n_b) == (2, 2, 3, 6)
    assert b.path_off.tolist() == [0, 2, 3] and b.path_ids.tolist() == [2, 3, 4]
    assert b.set_off.tolist() == [0, 1, 1, 2, 4] and b.set_ids.tolist() == [0, 1, 2, 5]
    with pytest.raises(ValueError, match="one read set per haplotype"):
        phasing.bubble_from_relevant(rel, 2, [[20]], [[[10]]])


class StandInRead:
    """What the reference's OrientedRead is to the methods at hand: hashable, with a length."""

    def __init__(self, ident, length):
        self.ident, self.length = ident, length

    def __len__(self):
        return self.length

    def __hash__(self):
        return hash(self.ident)

    def __eq__(self, other):
        return isinstance(other, StandInRead) and self.ident == other.ident

    def __repr__(self):
        return "read%d" % self.ident


class StandInMerged(StandInRead):
    prefix_lengths = [7]


class StandInGraph:
    edge_len = "weight"

    def __init__(self, exit_node, preds):
        self.exit_node, self.preds = exit_node, preds

    def predecessors_iter(self, node):
        return iter(self.preds)

    def __getitem__(self, pred):
        return {self.exit_node: {self.edge_len: self.preds[pred]}}


class StandInPhaser:
    """The attributes and methods of BubbleChainPhaser that the replaced methods touch."""

    def __init__(self, g):
        self.g = g
        self.prev_graph_reads = set()
        self.candidate_sets = []

    def get_all_reads(self, nodes):
        for node in nodes:
            yield node

    def branch(self, possible_paths, relevant_reads):
        raise AssertionError("not under test")

    def get_aligning_reads(self, nodes):
        raise AssertionError("the inherited method ran")

    def get_relevant_read_info(self, relevant_reads, cur_bubble_graph_reads, bubble_exit):
        raise AssertionError("the inherited method ran")


def test_device_phaser_with_an_index_on_a_stand_in_class():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "phasm"))
    try:
        import phasing_device
    finally:
        sys.path.pop(0)
    case = next(c for c in CASES if c["name"] == "bubble")
    q, ref = case["queries"][6], case["results"][6]                  # two preds, the minimum taken
    lengths = ru.lengths_of(case)
    reads = [StandInRead(i, int(n)) for i, n in enumerate(lengths)]
    host = phasing.HostIndex(lengths)
    index = host.phase_index(ru.rows_of(case))
    exit_node = reads[32]
    preds = {reads[p]: e for p, e in q["preds"]}
    preds[StandInMerged(1000, 500)] = 1                              # yields len(read): it is left out of the call
    cls = phasing_device.device_phaser(StandInPhaser, phasing.HostScorer(), index=index, read_id={r: r.ident for r in reads}, source=host)
    ph = cls(StandInGraph(exit_node, preds))
    ph.prev_graph_reads = {reads[x] for x in q["prev_graph"]}
    cur = [reads[x] for x in q["cur_graph"]]
    aligning = ph.get_aligning_reads(cur)
    assert sorted(r.ident for r in aligning) == list(ref["cur_aligning"])
    spanning = {reads[x] for x in q["prev_aligning"]} & aligning
    info = ph.get_relevant_read_info(spanning, set(cur), exit_node)
    assert sorted(r.ident for r in info) == list(ref["rel_reads"])
    for j, x in enumerate(ref["rel_reads"]):
        las, om = info[reads[x]]
        lo, hi = ref["aln_off"][j], ref["aln_off"][j + 1]
        assert om == ref["overlap_max"][j]
        assert [(b.ident, a0, a1) for b, a0, a1 in las] == list(zip(ref["aln_y"][lo:hi], ref["aln_a0"][lo:hi], ref["aln_a1"][lo:hi]))
    packed = phasing.pack_bubble([(reads[30], reads[20], reads[32]), (reads[30], reads[22], reads[24], reads[32])], [[set(), set()]], info)
    assert packed.n_reads == 3 and sorted(packed.overlap_max.tolist()) == sorted(ref["overlap_max"])
    assert ph.get_aligning_reads([]) == set() and ph.get_relevant_read_info(set(), set(cur), exit_node) == {}
    # without index and read_id nothing changes: the inherited methods stay
    plain = phasing_device.device_phaser(StandInPhaser, phasing.HostScorer())
    assert plain.get_aligning_reads is StandInPhaser.get_aligning_reads and plain.get_relevant_read_info is StandInPhaser.get_relevant_read_info
    with pytest.raises(ValueError, match="go together"):
        phasing_device.device_phaser(StandInPhaser, phasing.HostScorer(), index=index)
