"""The kernels of po_layout_superbubbles_all compiled for the HOST (tools/cyclic_host_emu.cpp: one lane per wave, threads one
after another) against the goldens, as a stand-alone program under AddressSanitizer + UBSan: the flat graph of every level,
the roots, the SCC stage and the superbubble stage on the flat graphs, the seeds of the discards, the merge, the cycle search
and the host's walk along its parents, the outputs -- with the host's caps and batches, checked without a GPU.  The edges go
in scrambled.  Every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import components_utils as cu
import cyclic_utils as cy
import emu_utils
from test_cyclic_oracle import CASES, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + ["tangle_3", "selfish_2", "ring_40", "lasso_70_6", "union_21_1"]
NO_NODE = 0xFFFFFFFF

emu = emu_utils.emu_fixture("cyclic")


def run_emu(emu, uv, order, n_total, perm):
    text = "%d %d %d\n" % (n_total, len(uv), len(order)) + "".join("%d %d\n" % tuple(uv[k]) for k in perm) + \
           " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_golden(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    stages = stage_inputs(c)
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    node = lambda s: np.asarray([cy.NONE if x == NO_NODE else x for x in ints(s)], np.int64)   # noqa: E731
    for r in c["results"]:
        edges, order, n_ids = stages[r["stage"]]
        uv = cu.uv_of(edges)
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(uv)).permutation(len(uv))
        lines = run_emu(emu, uv.tolist(), order, n_total, perm)
        assert len(lines) >= 6, lines[:1]
        n_order, n_bubbles, n_nested, n_cyclic, n_split, n_levels, n_rootless, n_runs, n_certified, n_filtered = ints(lines[0])
        batches, max_batch, most_levels, most_flat = ints(lines[1])
        table = np.asarray([ints(x) for x in lines[5].split(";") if x.strip()], dtype=np.int64).reshape(-1, 4)
        res = {"node_exit": node(lines[2]), "node_inside": node(lines[3]), "node_flags": np.asarray(ints(lines[4]), np.int64),
               "b_entrance": table[:, 0], "b_exit": table[:, 1], "b_inside": table[:, 2], "b_nested": table[:, 3],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_bubbles": n_bubbles, "n_nested": n_nested, "n_cyclic_bubbles": n_cyclic,
                         "n_split": n_split, "n_split_levels": n_levels, "n_rootless": n_rootless, "n_root_runs": n_runs,
                         "n_certified": n_certified, "n_edge_filtered": n_filtered}}
        cy.check_against_record(res, r)                                              # the golden: arrays, counts, run counts
        if n_order == 0:
            continue
        # the caps and the batches: no run took more levels than nodes + 2, a flat graph has at most twice the ranks, a batch
        # holds at most 8 rounds, every run has at least the closing batches of its level rounds and of its discard rounds
        assert most_levels == n_levels <= n_order + 2 and most_flat == n_order + n_split <= 2 * n_order
        assert max_batch <= 8 and batches >= 2 * n_runs


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    assert run_emu(emu, [(0, 2), (2, 4), (6, 0)], [0, 2], 8, [0, 1, 2])[0] == "invalid 2"
