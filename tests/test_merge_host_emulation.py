"""The kernels of po_layout_merge compiled for the HOST (tools/merge_host_emu.cpp: one lane per wave, threads one after
another) against the reference's goldens, with AddressSanitizer + UBSan: degrees and links, the pointer-jumping rounds,
the sort of the heads (handed over in scrambled order), the tables, the renamed edges and the ranks of the result,
checked without a GPU.  The edges go in scrambled.  The cycles of the direct cases (a self-loop, 2, 3, 64 and 65 nodes),
the ring and the lasso show that every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import emu_utils
import merge_utils as mu
import reduce_utils as ru
from test_merge_oracle import CASES, input_edges, node_lengths

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]


emu = emu_utils.emu_fixture("merge")


def run_emu(emu, e, order, lengths, n_nodes, perm):
    text = "%d %d %d\n" % (n_nodes, len(e), len(order)) + "".join("%d %d %d %d\n" % tuple(e[k]) for k in perm) + \
           " ".join(map(str, order)) + "\n" + " ".join(str(int(lengths[n])) for n in range(n_nodes)) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    L = node_lengths(c)
    for r in c["results"]:
        e = input_edges(c, r)
        perm = np.random.default_rng(len(e)).permutation(len(e))
        lines = run_emu(emu, e, r["order_before"], L, r["n_ids"], perm)
        if r["n_overflow"]:
            assert lines[0] == "overflow %d" % r["n_overflow"]          # the call fails; no wrapped weight is written
            continue
        assert len(lines) >= 8, lines[:2]
        ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
        flags = np.zeros(len(e), np.uint8)
        flags[perm] = np.frombuffer(lines[0].encode(), np.uint8) - 48
        assert np.array_equal(flags, ru.unpack_flags(r["flags"], len(e)))
        n_invalid, n_nodes, n_heads, n_merged, n_cycle, longest, n_self, n_over, n_kept, rounds = ints(lines[1])
        assert {"n_invalid": n_invalid, "n_nodes": n_nodes, "n_merged": n_heads, "n_nodes_merged": n_merged, "n_cycle_nodes": n_cycle,
                "max_path_nodes": longest, "n_self_loops": n_self, "n_overflow": n_over, "n_edges_out": n_kept,
                "n_edges_in": len(e)} == {k: r[k] for k in mu.STAT_KEYS}
        assert rounds <= r["rounds"] and (rounds > 0) == (r["n_merged"] > 0)
        want = mu.merge_paths(e[perm], r["order_before"], L, r["n_ids"])
        assert ints(lines[2]) == want["order"]
        for line, key in zip(lines[3:7], ("offsets", "members", "prefix", "lengths")):
            assert ints(line) == r[key].tolist(), key
        kept = [ints(x) for x in lines[7].split(";") if x]
        assert kept == want["edges"].tolist()                            # the kept edges, renamed, in input order
        assert ru.edge_digest(ru.sort_edges(np.asarray(kept, np.int64).reshape(-1, 4))) == r["kept_sha256"]
