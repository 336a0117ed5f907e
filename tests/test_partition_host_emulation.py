"""The kernels of po_layout_partition compiled for the HOST (tools/partition_host_emu.cpp: one lane per wave, threads one
after another) against the goldens, with AddressSanitizer + UBSan: the ranks, the trim rounds, the forward colouring, the
backward marking, the numbering of the roots, the table, the edge classes and the node flags, with the host's caps and
batches (scc_drive of partition.hip.h, which the library launches by), checked without a GPU.  The edges go in scrambled.
Every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import components_utils as cu
import emu_utils
import partition_utils as pu
from test_partition_oracle import CASES, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]


emu = emu_utils.emu_fixture("partition")


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
    for r in c["results"]:
        edges, order, n_ids = stages[r["stage"]]
        uv = cu.uv_of(edges)
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(uv)).permutation(len(uv))
        lines = run_emu(emu, uv.tolist(), order, n_total, perm)
        assert len(lines) >= 6, lines[:1]
        n_order, n_scc, n_single, max_n, max_e, n_self, *n_class = ints(lines[0])
        n_trimmed, outer, trim_rounds, fwd_rounds, bwd_rounds, batches, max_batch, beyond = ints(lines[1])
        edge_class = np.zeros(len(uv), np.int64)
        edge_class[perm] = ints(lines[4])
        table = np.asarray([ints(x) for x in lines[5].split(";") if x], dtype=np.int64).reshape(-1, 5)
        res = {"node_scc": np.asarray(ints(lines[2]), np.int64), "node_flags": np.asarray(ints(lines[3]), np.int64),
               "edge_class": edge_class, "first_node": table[:, 0], "n_nodes": table[:, 1], "n_edges": table[:, 2], "n_r_in": table[:, 3],
               "n_re_out": table[:, 4],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_sccs": n_scc, "n_nonsingleton_sccs": n_scc - n_single,
                         "n_singletons": n_single, "n_self_loops": n_self, "max_scc_nodes": max_n, "max_scc_edges": max_e,
                         "n_class": n_class}}
        weak = cu.weak_components(uv, order)
        pu.check_against_record(res, pu.reference_partitions(res, weak, uv, order), uv, r)
        want = pu.partition(uv, order)
        for k in pu.ARRAY_KEYS:
            assert np.array_equal(res[k], want[k]), k
        # the caps and the batch arithmetic: no phase was given more than its live nodes + 2 rounds, a batch holds at most 8
        # rounds, every phase ends within the batch of its closing round, and the emulation (threads one after another sees
        # every earlier store) needs no more rounds than the synchronous scheme
        assert n_trimmed == r["n_trimmed"] and beyond <= 2 and max_batch <= 8 and outer <= max(n_order, 0)
        assert (outer > 0) == (n_order > 0) and outer <= r["n_outer"]
        assert trim_rounds <= r["n_trim_rounds"] and fwd_rounds <= r["n_forward_rounds"] and bwd_rounds <= r["n_backward_rounds"]
        rounds = trim_rounds + fwd_rounds + bwd_rounds
        assert -(-rounds // 8) <= batches <= rounds // 8 + 3 * outer      # (at most one part-filled batch per phase)


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    assert run_emu(emu, [(0, 2), (2, 4), (6, 0)], [0, 2], 8, [0, 1, 2])[0] == "invalid 2"
