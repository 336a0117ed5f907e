"""The kernels of po_layout_bubblechains compiled for the HOST (tools/bubblechains_host_emu.cpp: one lane per wave, threads one
after another) against the goldens, with AddressSanitizer + UBSan: behind the ranks, the SCC stage and the superbubble
stage, the top-level entrances, their links and heads, the rounds to the outermost holder, the ranking rounds between two
buffer pairs, the sums, the filter, the table and the three arrays, with the host's caps and batches (round_phase of
components.hip.h, which the library launches by), checked without a GPU.  The edges go in scrambled.  Every loop is bounded:
a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import bubblechain_utils as bu
import components_utils as cu
import emu_utils
import superbubble_utils as su
from test_bubblechains_oracle import CASES, check_reference, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]
NO_NODE = 0xFFFFFFFF


emu = emu_utils.emu_fixture("bubblechains")


def run_emu(emu, uv, order, n_total, perm, min_nodes=1):
    text = "%d %d %d\n" % (n_total, len(uv), len(order)) + "".join("%d %d\n" % tuple(uv[k]) for k in perm) + \
           " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu, str(min_nodes)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_golden(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    stages = stage_inputs(c)
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    node = lambda s: np.asarray([bu.NONE if x == NO_NODE else x for x in ints(s)], np.int64)   # noqa: E731
    for r in c["results"]:
        edges, order, n_ids = stages[r["stage"]]
        uv = cu.uv_of(edges)
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(uv)).permutation(len(uv))
        lines = run_emu(emu, uv.tolist(), order, n_total, perm, r["min_nodes"])
        assert len(lines) >= 6, lines[:1]
        n_order, n_bubbles, n_nested, levels_f, n_top, n_heads, n_chains, n_short, chain_nodes, chain_edges, max_bubbles = ints(lines[0])
        nest_rounds, chain_rounds, batches, max_batch = ints(lines[1])
        table = np.asarray([ints(x) for x in lines[5].split(";") if x.strip()], dtype=np.int64).reshape(-1, 5)
        given = uv[perm] if len(uv) else uv
        res = {"node_chain": node(lines[2]), "node_bubble": node(lines[3]), "edge_chain": node(lines[4]),
               "c_first": table[:, 0], "c_last": table[:, 1], "c_bubbles": table[:, 2], "c_nodes": table[:, 3], "c_edges": table[:, 4],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_bubbles": n_bubbles, "n_top": n_top, "n_chains": n_chains,
                         "n_short": n_short, "n_chain_nodes": chain_nodes, "n_chain_edges": chain_edges, "max_chain_bubbles": max_bubbles}}
        bu.check_against_record(res, r, given)                                       # the golden
        check_reference(res, given, order, r)                                        # the reference's chains
        want = bu.scheme(given, order, r["min_nodes"], su.scheme(given, order))      # the restatement, on the edges as given
        for k in bu.ARRAY_KEYS:
            assert np.array_equal(res[k], want[k]), k
        if n_order == 0:
            continue
        # the caps and the batch arithmetic: a batch holds at most 8 rounds, every loop ends within the batch of its closing
        # round; the rounds stay within the logarithmic bounds (the emulation runs threads one after another: a thread of the
        # in-place holder rounds sees every earlier store, so it needs no more rounds than the synchronous scheme; the
        # ranking reads one buffer pair and writes the other, so it needs exactly as many)
        assert n_heads == n_chains + n_short and levels_f == r["n_levels_forward"]
        nest_bound, chain_bound = bu.round_bounds({"n_levels_forward": levels_f, "max_chain_bubbles": max_bubbles})
        assert max_batch <= 8
        assert nest_rounds <= r["n_nest_rounds"] <= nest_bound and (nest_rounds > 0) == (n_top > 0 and n_nested > 0)
        assert chain_rounds == r["n_chain_rounds"] <= chain_bound and (chain_rounds > 0) == (n_top > 0)
        rounds = nest_rounds + chain_rounds
        assert -(-rounds // 8) <= batches <= rounds // 8 + 2      # (at most one part-filled batch per loop)


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    assert run_emu(emu, [(0, 2), (2, 4), (6, 0)], [0, 2], 8, [0, 1, 2])[0] == "invalid 2"
