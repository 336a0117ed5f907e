"""The kernels of the ring election (phasm_amd/csrc/ringchains.hip.h) and the unchanged kernels of bubblechains.hip.h around
them, compiled for the HOST (tools/ringchains_host_emu.cpp: one lane per wave, threads one after another) against the goldens,
with AddressSanitizer + UBSan: behind the words that po_layout_superbubbles_all's stage leaves per rank (given here by
phasm_amd.cyclic.HostSuperbubblesAll, which tests/test_cyclic_host_emulation.py holds equal to that stage's own emulation),
the top-level entrances, their links and heads, the election's fixed number of rounds between its two buffer pairs, the
leaders, the ranking, the sums, the closing of the rings, the filter, the table and the three arrays, with the host's caps
and batches, checked without a GPU.  The edges go in scrambled.  Every loop is bounded: a subprocess that runs into its
timeout fails the test."""
import subprocess

import numpy as np
import pytest

import bubblechain_all_utils as ba
import bubblechain_utils as bu
import components_utils as cu
import emu_utils
from phasm_amd import cyclic
from test_bubblechains_all_oracle import CASES, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        [c["name"] for c in CASES if not c.get("direct") and any(r["n_ring_chains"] for r in c["results"])] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "ring_40", "lasso_70_6"]
NO_NODE = 0xFFFFFFFF

emu = emu_utils.emu_fixture("ringchains")


def run_emu(emu, uv, order, n_total, perm, min_nodes=1):
    given = [uv[k] for k in perm]
    host = cyclic.HostSuperbubblesAll(given, order)
    node_exit, node_inside, flags, _ = host.layout_superbubbles_all()
    st = host.superbubble_all_stats()
    rank = {int(x): r for r, x in enumerate(order)}
    word = lambda x: rank[int(x)] if int(x) != NO_NODE else NO_NODE   # noqa: E731
    text = "%d %d %d\n" % (n_total, len(uv), len(order)) + "".join("%d %d\n" % tuple(e) for e in given) + " ".join(map(str, order)) + "\n" + \
           "%d %d %d\n" % (st["n_bubbles"], st["n_nested"], st["n_cyclic_bubbles"]) + \
           "".join("%d %d %d\n" % (int(t) != NO_NODE, word(t), word(s)) for t, s in zip(node_exit.tolist(), node_inside.tolist()))
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
        edges, order, n_ids, _ = stages[r["stage"]]
        uv = cu.uv_of(edges)
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(uv)).permutation(len(uv))
        lines = run_emu(emu, uv.tolist(), order, n_total, perm, r["min_nodes"])
        assert len(lines) >= 6, lines[:1]
        n_order, n_top, n_path_heads, n_heads, n_chains, n_short, chain_nodes, chain_edges, max_bubbles, n_rings, ring_bubbles, ring_rounds = \
            ints(lines[0])
        nest_rounds, chain_rounds, batches, max_batch = ints(lines[1])
        table = np.asarray([ints(x) for x in lines[5].split(";") if x.strip()], dtype=np.int64).reshape(-1, 5)
        given = uv[perm] if len(uv) else uv
        res = {"node_chain": node(lines[2]), "node_bubble": node(lines[3]), "edge_chain": node(lines[4]),
               "c_first": table[:, 0], "c_last": table[:, 1], "c_bubbles": table[:, 2], "c_nodes": table[:, 3], "c_edges": table[:, 4],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_bubbles": r["n_bubbles"], "n_top": n_top, "n_chains": n_chains,
                         "n_short": n_short, "n_chain_nodes": chain_nodes, "n_chain_edges": chain_edges, "max_chain_bubbles": max_bubbles,
                         "n_ring_chains": n_rings, "n_ring_bubbles": ring_bubbles, "n_cyclic_bubbles": r["n_cyclic_bubbles"]}}
        ba.check_against_record(res, r, given)                                       # the golden
        want = ba.scheme(given, order, r["min_nodes"])                               # the restatement, on the edges as given
        for k in ba.ARRAY_KEYS:
            assert np.array_equal(res[k], want[k]), k
        if n_order == 0:
            continue
        # the caps and the fixed round count: heads and leaders add up, the election ran exactly ceil(log2 n_top) + 1 rounds
        # where a bubble lies in an SCC and not at all elsewhere, a batch holds at most 8 rounds, and the ranking -- which
        # reads one buffer pair and writes the other, so the emulation needs exactly the synchronous rounds -- stays within
        # its logarithmic bound although a ring gives it no head of its own
        assert n_heads == n_path_heads + n_rings == n_chains + n_short
        assert ring_rounds == r["n_ring_rounds"] == (bu.log2_ceil(n_top) + 1 if n_top and r["n_cyclic_bubbles"] else 0)
        assert max_batch <= 8 and (chain_rounds > 0) == (n_top > 0)
        assert chain_rounds <= bu.log2_ceil(max(max_bubbles, 2)) + 2
        rounds = nest_rounds + chain_rounds
        assert -(-rounds // 8) <= batches <= rounds // 8 + 2      # (at most one part-filled batch per loop)


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    text = "8 3 2\n0 2\n2 4\n6 0\n0 2\n0 0 0\n0 4294967295 4294967295\n0 4294967295 4294967295\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split("\n")[0] == "invalid 2"
