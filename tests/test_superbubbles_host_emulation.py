"""The kernels of po_layout_superbubbles compiled for the HOST (tools/superbubbles_host_emu.cpp: one lane per wave, threads one
after another) against the goldens, with AddressSanitizer + UBSan: behind the ranks and the SCC stage, the degrees and the
lists of D, the level rounds, the two trees level by level, the pairs, the enclosing bubbles, the discards, the labels, the
sums and the table, with the host's caps and batches (round_phase of components.hip.h, which the library launches by),
checked without a GPU.  The edges go in scrambled.  Every loop is bounded: a subprocess that runs into its timeout fails
the test."""
import subprocess

import numpy as np
import pytest

import components_utils as cu
import emu_utils
import superbubble_utils as su
from test_superbubbles_oracle import CASES, check_reference, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]
NO_NODE = 0xFFFFFFFF


emu = emu_utils.emu_fixture("superbubbles")


def run_emu(emu, uv, order, n_total, perm):
    text = "%d %d %d\n" % (n_total, len(uv), len(order)) + "".join("%d %d\n" % tuple(uv[k]) for k in perm) + \
           " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_golden(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    stages = stage_inputs(c)
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    node = lambda s: np.asarray([su.NONE if x == NO_NODE else x for x in ints(s)], np.int64)   # noqa: E731
    for r in c["results"]:
        edges, order, n_ids = stages[r["stage"]]
        uv = cu.uv_of(edges)
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(uv)).permutation(len(uv))
        lines = run_emu(emu, uv.tolist(), order, n_total, perm)
        assert len(lines) >= 6, lines[:1]
        n_order, n_scc, n_real, p_nodes, p_edges, n_bubbles, n_nested, n_loops, n_discarded, levels_f, levels_b = ints(lines[0])
        level_rounds, discard_rounds, batches, max_batch, beyond, per_level = ints(lines[1])
        table = np.asarray([ints(x) for x in lines[5].split(";") if x.strip()], dtype=np.int64).reshape(-1, 4)
        res = {"node_exit": node(lines[2]), "node_inside": node(lines[3]), "node_flags": np.asarray(ints(lines[4]), np.int64),
               "b_entrance": table[:, 0], "b_exit": table[:, 1], "b_inside": table[:, 2], "b_nested": table[:, 3],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_p_nodes": p_nodes, "n_p_edges": p_edges, "n_bubbles": n_bubbles,
                         "n_nested": n_nested, "n_self_loop_nodes": n_loops, "n_discarded": n_discarded}}
        if n_order == 0:
            res["stats"].update({"n_p_nodes": 0, "n_p_edges": 0})
        su.check_against_record(res, r)                                              # the golden
        check_reference(res, su.node_sets(res, order), uv, order, r)                 # the reference's pairs and node sets
        want = su.scheme(uv, order)
        for k in su.ARRAY_KEYS:
            assert np.array_equal(res[k], want[k]), k
        if n_order == 0:
            continue
        # the caps and the batch arithmetic: no loop was given more than its live nodes + 2 rounds, a batch holds at most 8
        # rounds, every loop ends within the batch of its closing round; forward and backward levels rise in the same
        # rounds, and the emulation (threads one after another: a thread sees every earlier store) needs no more rounds than
        # the synchronous scheme; the launches per level: one per level of each tree, one per forward level for the
        # enclosing bubbles, and one more per forward level where a bubble is nested
        assert (levels_f, levels_b) == (r["n_levels_forward"], r["n_levels_backward"]) and levels_f <= n_real <= n_order
        assert beyond <= 2 and max_batch <= 8
        assert 1 <= level_rounds <= max(levels_f, 1) + 1 and 2 * level_rounds <= r["n_level_rounds"] + 2
        assert discard_rounds <= r["n_discard_rounds"] and (discard_rounds > 0) == (n_loops > 0)
        rounds = level_rounds + discard_rounds
        assert -(-rounds // 8) <= batches <= rounds // 8 + 2      # (at most one part-filled batch per loop)
        assert per_level == 2 * levels_f + levels_b + (levels_f if n_nested else 0)


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    assert run_emu(emu, [(0, 2), (2, 4), (6, 0)], [0, 2], 8, [0, 1, 2])[0] == "invalid 2"
