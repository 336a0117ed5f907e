"""The kernels of po_phase_paths compiled for the HOST (tools/paths_host_emu.cpp: one lane per wave, threads one after
another) against the goldens, with AddressSanitizer + UBSan: behind the ranks, the SCC stage, the superbubble stage and the
bubble-chain stage, the bubbles numbered by (chain, position), the sorted keys of the edges, the counting rounds with the
host's cap and batches (round_phase of components.hip.h, which the library launches by), the table, the offsets, the
predecessors, the interior and both passes of the walk of every listed path, the saturating case included, checked without a
GPU.  Every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import emu_utils
import paths_utils as pp
from test_paths_oracle import BY_NAME, CASES

emu = emu_utils.emu_fixture("paths")


def run_emu(emu, order, edges, max_paths, n_total=None):
    n_total = max([int(x) + 1 for x in order] + [1]) if n_total is None else n_total
    text = "%d %d %d\n" % (n_total, len(edges), len(order)) + "".join("%d %d %d\n" % tuple(e) for e in edges) + \
           " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu, str(max_paths)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


def result_of_lines(lines):
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    head = ints(lines[0])
    table = [ints(x) for x in lines[1].split(";") if x.strip()]
    res = {k: np.asarray([row[i] for row in table], dtype=np.uint64 if k == "b_paths" else np.int64) for i, k in enumerate(pp.TABLE_KEYS)}
    for k, ln in zip(pp.CSR_KEYS, lines[2:10]):
        res[k] = np.asarray(ints(ln), dtype=np.int64)
    keys = ("n_bubbles", "n_stray_edges", "n_bare", "n_unlisted", "n_saturated", "n_listed_paths", "n_path_nodes", "max_paths_seen",
            "max_path_nodes", "n_count_rounds", "n_batches", "max_batch")
    res["stats"] = dict(zip(keys, head))
    return res


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_compiled_kernels_equal_the_golden(emu, case):
    order, edges, max_paths = pp.case_inputs(case)
    lines = run_emu(emu, order, edges, max_paths)
    assert len(lines) >= 10, lines[:1]
    got = result_of_lines(lines)
    want = pp.result_of_record(case["result"])
    got["stats"].update({"n_nodes": len(order), "n_edges": len(edges)})
    pp.same(got, want)
    st = got["stats"]
    assert st["n_stray_edges"] == 0 and st["n_count_rounds"] == want["stats"]["n_count_rounds"]
    if len(want["b_entrance"]):
        # the cap and the batch arithmetic: a batch holds at most 8 rounds, the loop ends within the batch of its closing round
        assert st["n_count_rounds"] <= int(want["b_inside"].max()) + 2 and st["max_batch"] <= 8
        assert -(-st["n_count_rounds"] // 8) <= st["n_batches"] <= st["n_count_rounds"] // 8 + 1


def test_the_edges_in_another_order_change_the_order_of_the_paths_only(emu):
    order, edges, max_paths = pp.case_inputs(BY_NAME["direct_su_sb_random_dag_200_seed3"])
    perm = np.random.default_rng(5).permutation(len(edges))
    given = [edges[k] for k in perm]
    got = result_of_lines(run_emu(emu, order, given, max_paths))
    want = pp.scheme(given, order, max_paths)                       # the restatement, on the edges as given
    for k in pp.ARRAY_KEYS:
        assert np.array_equal(got[k], want[k]), k
    base = pp.result_of_record(BY_NAME["direct_su_sb_random_dag_200_seed3"]["result"])
    for k in pp.TABLE_KEYS + ("inside_off", "inside_nodes", "pred_off", "bubble_path_off"):
        assert np.array_equal(got[k], base[k]), k


def test_capacity_and_an_edge_end_outside_the_node_order(emu):
    order, edges, _ = pp.case_inputs(BY_NAME["direct_unlisted_62"])
    assert run_emu(emu, order, edges, 2**62 + 1)[0] == "capacity paths"
    order, edges, _ = pp.case_inputs(BY_NAME["direct_saturated_64"])
    got = result_of_lines(run_emu(emu, order, edges, 2**64 - 1))     # saturated implies unlisted whatever max_paths says
    assert got["b_flags"].tolist() == [pp.UNLISTED | pp.SATURATED] and got["stats"]["n_listed_paths"] == 0
    assert run_emu(emu, [0, 2], [(0, 2, 5), (2, 4, 5), (6, 0, 5)], 4, n_total=8)[0] == "invalid 2"
