"""The kernels of po_layout_coverage compiled for the HOST (tools/coverage_host_emu.cpp: one lane per wave, threads one
after another) against the reference's goldens, with AddressSanitizer + UBSan: node_of, the pair table and its bounded
probes, the sums, the lists and inclusion-exclusion per edge, checked without a GPU.  The rows go in scrambled.  A
subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import coverage_utils as cu
import emu_utils
from test_coverage_oracle import CASES, application

NAMES = ["_".join(str(v) for v in s.values()) for s in cu.NEW_CASES] + \
        ["tangle_11", "selfish_2", "reduced_hub_1025", "reduced_line_101", "union_21_1", "ring_40", "lasso_12_8", "lasso_70_6"]


emu = emu_utils.emu_fixture("coverage")


def run_emu(emu, rows, e, members, L, n_ids):
    K = len(L) - n_ids
    paths = [members[n_ids + k] for k in range(K)]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    text = "%d %d %d %d %d\n" % (n_ids, K, offsets[-1], len(e), len(rows)) + " ".join(str(int(x)) for x in L[:n_ids]) + "\n" + \
           " ".join(map(str, offsets[:-1].tolist())) + "\n" + " ".join(str(int(x)) for x in L[n_ids:]) + "\n" + \
           " ".join(str(m) for p in paths for m in p) + "\n" + "".join("%d %d %d\n" % (u, v, w) for u, v, w, _ in e) + \
           "".join("%d %d\n" % (a, b) for a, b in rows)
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    for r in c["results"]:
        rows, e, members, L = application(c, r)
        pairs = np.asarray(rows, dtype=np.int64).reshape(-1, 6)[:, :2]
        pairs = pairs[np.random.default_rng(len(pairs)).permutation(len(pairs))]
        lines = run_emu(emu, pairs.tolist(), e.tolist(), members, L, r["n_ids"])
        if len(e) == 0:                                                       # (run_coverage returns before any launch)
            continue
        assert [int(x) for x in lines[0].split()] == [r["n_nodes"], r["n_pairs"], r["max_set"], 0], lines[0]
        got = np.asarray([[int(x) for x in l.split()] for l in lines[1:1 + len(e)]], dtype=np.int64).reshape(-1, 2)
        cu.check_record(r, e[:, 0], e[:, 1], got[:, 0], got[:, 1], got[:, 0].astype(np.float64) / got[:, 1].astype(np.float64))


def test_the_zero_length_quirk_a_zero_path_and_invalid_input(emu):
    rows = [(0, 2), (2, 4), (6, 0), (2, 2)]
    L = [100, 100, 0, 0, 50, 50, 70, 70]
    e = [(0, 2, 30, 1), (2, 4, 5, 1), (2, 2, 7, 1), (4, 2, 0, 1)]
    lines = run_emu(emu, rows, e, {}, L, len(L))
    want = cu.edge_coverage_by_sets([r + (0, 0, 0, 0) for r in rows], e, {}, L)
    assert [int(x) for x in lines[0].split()][3] == 1                         # one edge with path_length == 0
    got = [[int(x) for x in l.split()] for l in lines[1:5]]
    assert [g[0] for g in got] == want[0].tolist() and [g[1] for g in got] == want[1].tolist() == [30, 55, 7, 0]
    assert run_emu(emu, rows, [(0, 9, 1, 1)], {}, L, len(L))[0] == "invalid 1"    # an edge that names no node
    assert run_emu(emu, [(0, 8)], e, {}, L, len(L))[0] == "invalid 1"             # a row that names no read
