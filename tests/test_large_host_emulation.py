"""The kernels of po_phase_large compiled for the host (tools/large_host_emu.cpp: one lane per wave, one thread per workgroup,
AddressSanitizer + UBSan) against tests/golden/large_cases.npz: the best list exactly, every score within ``table_tol`` of the
reference's.  With one thread the sum runs in read order, the order of ``large_utils.definition``: its scores are the
reference's bit for bit.  A refused call ends the program with status 1."""
import subprocess

import pytest

import emu_utils
import large_utils as lu
from phasm_amd import phasing

emu = emu_utils.emu_fixture("large")
CASES = lu.cases()


def emu_input(case, n_best=None, n_reads=None, bad_id=False):
    hp, rel, reads_of = lu.host_paths(case), lu.rel_of(case), lu.reads_of_node(case)
    b = case["bubble"]
    inside, paths = hp.interior_of(b), hp.paths_of(b)
    node_off, node_ids = phasing.large_node_lists(rel, inside, reads_of)
    order, _ = lu.graph_inputs(case)
    off = [0]
    for p in paths:
        off.append(off[-1] + len(p))
    R = len(case["overlap_max"]) if n_reads is None else n_reads
    ids = node_ids.tolist()
    if bad_id:
        ids[0] = len(case["b_reads"])
    nums = [max(order) + 1, len(inside), len(paths), R, len(case["b_reads"]), case["ploidy"] if n_best is None else n_best]
    for part in (inside, off, [x for p in paths for x in p], case["overlap_max"], case["aln_off"], case["aln_b"], case["aln_a0"], case["aln_a1"],
                 node_off.tolist(), ids):
        nums += list(part)
    return " ".join(str(int(x)) for x in nums)


def run_emu(emu, text):
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout, out.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_compiled_kernels_equal_the_reference(emu, case):
    code, out, err = run_emu(emu, emu_input(case))
    assert code == 0, err[-2000:]
    head, best_line, score_line = out.split("\n")[:3]
    n, longest = (int(x) for x in head.split())
    best = [(int(e.split()[0]), float.fromhex(e.split()[1])) for e in best_line.split(";") if e.strip()]
    scores = [float.fromhex(x) for x in score_line.split()]
    lu.check_scores(scores, case)
    assert scores == case["ref"]["scores"]                      # (one thread: the reference's order of additions)
    assert [p for p, _ in best] == case["ref"]["best"] and n == len(best) == min(case["ploidy"], len(scores))
    assert [s for _, s in best] == [scores[p] for p, _ in best]
    assert longest == max(len(p) for p in lu.host_paths(case).paths_of(case["bubble"]))


def test_a_refused_call_ends_with_status_1(emu):
    case = CASES[0]
    for text in (emu_input(case, n_best=0), emu_input(case, n_best=9), emu_input(case, n_reads=0), emu_input(case, bad_id=True),
                 emu_input(case)[:40]):
        code, out, _ = run_emu(emu, text)
        assert code == 1 and out == ""
