"""The kernels of po_phase_branch compiled for the HOST (tools/phase_host_emu.cpp: one lane per wave, one thread per workgroup,
threads one after another) against the goldens, with AddressSanitizer + UBSan: the bitsets, the intervals, the table tile by
tile, the digits of an extension id, the start-of-block test, the multinomial, the filter, the places, the level histogram and
the survivors, launched as run_phase of c_api.hip launches them, checked without a GPU.  The program is a stand-alone
executable run as a subprocess; every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import pytest

import emu_utils
import phase_utils as pu
from phasm_amd import phasing

CASES = pu.load_golden()["cases"]


emu = emu_utils.emu_fixture("phase")


def run_emu(emu, case, pruned):
    pr = case["prune"] if pruned else None
    levels = phasing.prune_levels(pr["factor"], pr["step"], pr["max_rounds"]) if pr else []
    head = [case["k"], case["P"], case["C"], case["R"], case["n_b"], case["start"], case["min_span"], int(pr is not None),
            pr["max_candidates"] if pr else 0, len(levels)]
    text = " ".join(map(str, head)) + " %r\n" % case["threshold"] + \
           "".join(" ".join(map(str, case[key])) + "\n" for key in pu.INPUT_KEYS) + " ".join(x.hex() for x in levels) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert len(lines) >= 4, lines[:1]
    entries = lambda s: [(int(c), int(e), float.fromhex(r)) for c, e, r in (x.split() for x in s.split(";") if x.strip())]  # noqa: E731
    return [int(x) for x in lines[0].split()], entries(lines[1]), entries(lines[2]), [float.fromhex(x) for x in lines[3].split()]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_host_compiled_kernels_equal_the_golden(emu, name):
    case = next(c for c in CASES if c["name"] == name)
    ref = case["ref"]
    (n_ext, n_kept, n_out, _), kept, same, table = run_emu(emu, case, False)
    assert same == kept and n_kept == n_out == len(kept)
    got = {"kept_cand": [x[0] for x in kept], "kept_ext": [x[1] for x in kept], "kept_rl": [x[2] for x in kept]}
    (_, _, n_left, level_used), kept2, left, _ = run_emu(emu, case, True)
    assert kept2 == kept and n_left == len(left)
    place = {(c, e): j for j, (c, e, _) in enumerate(kept)}
    got["surv"] = [place[(c, e)] for c, e, _ in left]
    assert [x[2] for x in left] == [got["kept_rl"][j] for j in got["surv"]]
    k, P, R = case["k"], case["P"], case["R"]
    got["scores"], got["winner"] = None, None
    if R:
        # the paths' own scores are the table rows of the candidate without reads (candidate 0 of every case, slot 0)
        assert case["set_off"][1] == 0
        got["scores"] = [table[p] / R for p in range(P)]
        got["winner"] = phasing.best_paths(got["scores"], 1)[0]
    pu.check_result(got, ref, case)
    full, listed = pu.scheme_all_rl(case)
    assert n_ext == case["C"] * int(listed.sum())
    want = phasing.HostScorer().table(pu.bubble_of(case)).reshape(-1)
    assert len(table) == len(want) and all(abs(g - w) <= pu.table_tol(w, R) for g, w in zip(table, want))
    assert level_used == (len(ref["levels"]) - 1 if ref["levels"] else -1)


def test_a_call_the_library_refuses_ends_the_program(emu):
    out = subprocess.run([emu], input="9 1 1 0 1 0 0 0 0 0 0.0\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 1
