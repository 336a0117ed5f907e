"""The kernels of po_phase_index and po_phase_relevant compiled for the HOST (tools/relevant_host_emu.cpp: one lane per wave, one
thread per workgroup, threads one after another) against the goldens, with AddressSanitizer + UBSan: the claim of a key and
the winner by sequence number, the fill, the sort by rank, the places, the bitsets and their rank queries, the counted and
written alignments, the look-ups of overlap_max, launched as c_api.hip launches them, checked without a GPU.  The program is a
stand-alone executable run as a subprocess; every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import pytest

import emu_utils
import relevant_utils as ru

CASES = ru.load_golden()["cases"]

emu = emu_utils.emu_fixture("relevant")


def run_emu(emu, case, n_slots=0):
    rows = ru.rows_of(case)
    text = ["%d %d %d %d" % (2 * case["n_seg"], len(rows), n_slots, len(case["queries"])), " ".join(map(str, ru.lengths_of(case).tolist())),
            " ".join(map(str, rows.reshape(-1).tolist()))]
    for q in case["queries"]:
        text.append("%d %d %d %d %d %d" % (q["mode"], q["min_span"], len(q["cur_graph"]), len(q["prev_graph"]), len(q["prev_aligning"]),
                                           len(q["preds"])))
        for l in (q["cur_graph"], q["prev_graph"], q["prev_aligning"], [p[0] for p in q["preds"]], [p[1] for p in q["preds"]]):
            text.append(" ".join(map(str, l)))
    out = subprocess.run([emu], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    assert len(lines) >= 3 + 9 * len(case["queries"]), lines[:4]
    head, off, flat = ints(lines[0]), ints(lines[1]), ints(lines[2])
    entries = [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]
    results = []
    for i in range(len(case["queries"])):
        blk = [ints(s) for s in lines[3 + 9 * i:12 + 9 * i]]
        sizes, ca, rel, om, aln_off, aln_b, a0, a1, b = blk
        assert sizes == [len(ca), sizes[1], sizes[2], len(rel), len(aln_b), len(b)] and len(om) == len(rel) and len(aln_off) == len(rel) + 1
        assert all(x < len(b) for x in aln_b)
        results.append({"cur_aligning": ca, "n_spanning": sizes[1], "fell_back": sizes[2], "rel_reads": rel, "overlap_max": om,
                        "aln_off": aln_off, "aln_y": [b[x] for x in aln_b], "aln_a0": a0, "aln_a1": a1, "b_reads": b})
    return head, off, entries, results


def check(case, head, off, entries, results):
    want_off, want = ru.golden_index(case)
    assert off == [int(v) for v in want_off] and entries == [tuple(int(v) for v in w) for w in want]
    deg = [off[x + 1] - off[x] for x in range(len(off) - 1)]
    assert head == [len(want), max(deg + [0]), 0]
    for i, (got, ref) in enumerate(zip(results, case["results"])):
        ru.same_result(got, ref, "%s q%d" % (case["name"], i))


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_host_compiled_kernels_equal_the_golden(emu, name):
    case = next(c for c in CASES if c["name"] == name)
    check(case, *run_emu(emu, case))


def test_probing_wraps_past_the_end_of_a_small_table(emu):
    """A table with ONE slot more than there can be keys: the probe sequences run past the table's end and start again at
    slot 0, in the claim, in the places and in the look-ups of overlap_max."""
    case = next(c for c in CASES if c["name"] == "bubble")
    check(case, *run_emu(emu, case, n_slots=2 * len(ru.rows_of(case)) + 1))


def test_a_row_outside_the_reads_is_counted(emu):
    out = subprocess.run([emu], input="4 2 0 0\n9 9 9 9\n0 1 1 2 3 4\n2 4 1 2 3 4\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split("\n")[0].split()[2] == "1"
