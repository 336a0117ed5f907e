"""The kernels of po_layout_diamonds compiled for the HOST (tools/diamond_host_emu.cpp: one lane per wave, threads one
after another) against the reference's goldens, with AddressSanitizer + UBSan: degrees and in-edge ids, footprints, the
rounds with the candidates handed over in scrambled order and the node pass, checked without a GPU.  The direct cases
bring what no GFA case of the file has: node 0 as pred1, self-loops on a gt1, a predecessor that is the end node's own
mirror, fans that settle one end node per round."""
import subprocess

import numpy as np
import pytest

import emu_utils
import reduce_utils as ru
from test_diamond_oracle import CASES, GOLDEN, input_edges

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_129", "reduced_hub_1025", "reduced_stagger_1100"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]


emu = emu_utils.emu_fixture("diamond")


def run_emu(emu, e, order, perm):
    n_nodes = int(max([0] + order + e[:, :2].reshape(-1).tolist())) + 3
    text = "%d %d %d\n" % (n_nodes, len(e), len(order)) + "".join("%d %d\n" % (e[k, 0], e[k, 1]) for k in perm) + \
           " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert len(lines) >= 3, out.stdout[:200]
    flags = np.zeros(len(e), np.uint8)
    flags[perm] = np.frombuffer(lines[0].encode(), np.uint8) - 48
    return flags, [int(x) for x in lines[1].split()], [int(x) for x in lines[2].split()]


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    for r in c["results"]:
        e = input_edges(c, r)
        perm = np.random.default_rng(len(e)).permutation(len(e))
        flags, (n_invalid, n_cand, n_diamonds, n_nodes, n_removed, n_kept, rounds), left = run_emu(emu, e, r["order_before"], perm)
        assert np.array_equal(flags, ru.unpack_flags(r["flags"], len(e)))
        assert left == r["order_left"]
        assert (n_invalid, n_cand, n_diamonds, n_nodes, n_removed, n_kept) == \
               (0, r["n_candidates"], r["n_diamonds"], r["n_nodes"], 2 * r["n_diamonds"], r["n_kept"])
        assert (rounds > 0) == (n_cand > 0) and rounds <= GOLDEN["branch_totals"]["max_rounds"]
        # (threads one after another and marks never reset: the emulation may need fewer rounds than the restatement, never more)
        assert rounds <= r["rounds"]
