"""po_phase_index and po_phase_relevant on the device against tests/golden/relevant_cases.npz (the reference's own
get_aligning_reads, get_relevant_read_info and _get_max_possible_overlap on its own mapping): every golden case through the C
ABI, exact equality throughout; the index built and copied out twice with equal bytes; the chain index -> gather -> bubble ->
po_phase_branch against pack_bubble -> po_phase_branch on three phase goldens; one union of disjoint copies of the small cases
with more than 530 000 rows -- past one capped grid of 524 288 threads and past the one-launch scan -- queried in its first, a
middle and its last copy."""
import numpy as np
import pytest

import phase_utils as pu
import relevant_utils as ru
from phasm_amd import phasing
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

CASES = ru.load_golden()["cases"]


def indexed(lengths, rows):
    ov = ExactOverlapper()
    ru.add_reads(ov, lengths)
    res = ov.result_from_rows(ru.rows_array(rows))
    index = ov.phase_index(res)
    res.free()                                   # the index stays valid without the rows
    return ov, index


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_the_golden(name):
    case = next(c for c in CASES if c["name"] == name)
    ov, index = indexed(case["lengths"], ru.rows_of(case))
    want_off, want = ru.golden_index(case)
    st = ov.phase_index_stats()
    deg = np.diff(np.asarray(want_off, dtype=np.int64))
    assert (st["n_rows"], st["n_keys"], st["max_degree"], st["n_invalid"]) == (len(ru.rows_of(case)), len(want), int(deg.max()), 0)
    assert len(index) == 0
    off, entries = ov.phase_index_entries(index)
    ru.same_index(off, entries, want_off, want)
    # a second build, a second copy: the same bytes
    res = ov.result_from_rows(ru.rows_array(ru.rows_of(case)))
    again = ov.phase_index(res)
    off2, entries2 = ov.phase_index_entries(again)
    assert off2.tobytes() == off.tobytes() and entries2.tobytes() == entries.tobytes()
    again.free()
    res.free()
    for i, (q, ref) in enumerate(zip(case["queries"], case["results"])):
        got = ru.query_source(ov, index, q)
        ru.same_result(got, ref, "%s q%d" % (name, i))
        st = ov.relevant_stats()
        assert (st["n_cur_aligning"], st["n_spanning"], st["fell_back"], st["n_relevant"], st["n_alignments"], st["n_b"]) == (
            len(ref["cur_aligning"]), ref["n_spanning"], ref["fell_back"], len(ref["rel_reads"]), len(ref["aln_y"]), len(ref["b_reads"]))
        if i == 0:
            assert ru.query_source(ov, index, q) == got
    index.free()
    ov.close()


def test_rows_outside_the_reads_fail_the_index():
    ov = ExactOverlapper()
    ru.add_reads(ov, [50, 50])
    res = ov.result_from_rows(ru.rows_array([(0, 1, 1, 2, 3, 4), (2, 4, 1, 2, 3, 4), (7, 0, 1, 2, 3, 4)]))
    with pytest.raises(ValueError, match="po_phase_index: a row names a read the handle does not hold"):
        ov.phase_index(res)
    assert ov.phase_index_stats()["n_invalid"] == 2
    empty = ov.result_from_rows(ru.rows_array([]))
    index = ov.phase_index(empty)                      # no rows: an index without keys
    off, entries = ov.phase_index_entries(index)
    assert off.tolist() == [0] * 5 and len(entries) == 0
    rel = ov.phase_relevant(index, [3, 1, 3], [0], [1], [(2, 9)], 0, 1)
    assert rel.cur_aligning.tolist() == [1, 3] and rel.rel_reads.tolist() == [1] and rel.overlap_max.tolist() == [50]
    assert rel.b_reads.tolist() == [0, 1, 3] and rel.aln_off.tolist() == [0, 0]
    ov.add_segment("late", 10)
    with pytest.raises(ValueError, match="reads were added to the handle after the index was built"):
        ov.phase_relevant(index, [1])
    for r in (index, empty, res):
        r.free()
    ov.close()


@pytest.mark.parametrize("pc", ru.chain_cases(), ids=lambda pc: pc["name"])
def test_the_chain_on_the_device(pc):
    x = ru.phase_case_as_rows(pc)
    ov, index = indexed(x["lengths"], x["rows"])
    rel = phasing.relevant_reads(ov, index, x["cur_graph"], [], x["prev_aligning"], x["preds"], False, pc["min_span"])
    assert not rel.fell_back and rel.rel_reads.tolist() == x["prev_aligning"] and rel.overlap_max.tolist() == list(pc["overlap_max"])
    bubble = phasing.bubble_from_relevant(rel, pc["k"], x["paths"], x["read_sets"])
    got = pu.result_of(ov, ru.chained_case(pc, bubble))
    pu.check_result(got, pc["ref"], pc)
    relevant = {int(r): (rel.alignments_of(j), int(rel.overlap_max[j])) for j, r in enumerate(rel.rel_reads)}
    packed = phasing.pack_bubble([("in", *p, "out") for p in x["paths"]], x["read_sets"], relevant, expand=lambda node: (node,))
    want = pu.result_of(ov, ru.chained_case(pc, packed))
    assert got["kept_cand"] == want["kept_cand"] and got["kept_ext"] == want["kept_ext"] and got["surv"] == want["surv"]
    assert all(pu.same_rl(g, w, pc["k"], pc["R"]) for g, w in zip(got["kept_rl"], want["kept_rl"]))
    index.free()
    ov.close()


def test_past_one_grid_and_one_scan_window():
    per_copy = sum(len(ru.rows_of(c)) for c in CASES)
    n_copies = -(-530000 // per_copy)
    lengths, rows, shifts = ru.union_case(CASES, n_copies)
    assert len(rows) >= 530000 and 2 * len(lengths) > 64 * 4096            # rows past one grid, reads past the one-launch scan
    ov, index = indexed(lengths, rows)
    st = ov.phase_index_stats()
    assert st["n_rows"] == len(rows) and st["n_keys"] == n_copies * sum(len(c["index_b"]) for c in CASES) and st["max_degree"] == 2049
    maps = [ru.mapping(c) for c in CASES]
    for copy in (0, n_copies // 2, n_copies - 1):
        for ci, case in enumerate(CASES):
            shift = shifts[copy * len(CASES) + ci]
            for qi in (0, len(case["queries"]) - 1, 1):
                q = case["queries"][qi]
                want = ru.shifted_result(ru.definition(case, q, maps[ci]), shift)
                ru.same_result(ru.query_source(ov, index, ru.shifted_query(q, shift)), want, "copy %d %s q%d" % (copy, case["name"], qi))
    # the entries of the last copy's last case, shifted back, are the small case's
    off, entries = ov.phase_index_entries(index)
    case, shift = CASES[-1], shifts[-1]
    want_off, want = ru.golden_index(case)
    lo = int(off[shift])
    assert (off[shift:].astype(np.int64) - lo).tolist() == [int(v) for v in want_off]
    tail = entries[lo:]
    seq_shift = 2 * (len(rows) - len(ru.rows_of(case)))
    assert [(int(b) - shift, int(a0), int(a1), int(s) - seq_shift) for b, a0, a1, s in tail.tolist()] == [tuple(int(v) for v in w) for w in want]
    index.free()
    ov.close()
