"""The kernels of po_layout_tips compiled for the HOST (tools/tips_host_emu.cpp: one lane per wave, threads one after
another) against the reference's goldens, with AddressSanitizer + UBSan: degrees and id sums, the rounds of both tip
passes with the candidates handed over in scrambled order, the hash table of the symmetry pass and the node pass,
checked without a GPU.  The direct cases bring what no GFA case of the file has: weights <= 0, self-loops, the edge (a, a^1), 2-cycles."""
import subprocess

import numpy as np
import pytest

import emu_utils
import reduce_utils as ru
import tips_utils as tu
from test_tips_oracle import CASES, input_edges

NAMES = [c["name"] for c in CASES if c.get("direct") or "synth" in c] + \
        ["reduced_" + n for n in ("ladder_varlen", "cfg2_1k", "layout_random_1008", "line_109", "hub_129", "hub_1025", "stagger_1100", "tie_8")]


emu = emu_utils.emu_fixture("tips")


def run_emu(emu, e, order, L, B, perm):
    n_nodes = int(max([0] + order + e[:, :2].reshape(-1).tolist())) + 3
    text = "%d %d %d %d %d\n" % (n_nodes, L, B, len(e), len(order)) + \
           "".join("%d %d %d\n" % (e[k, 0], e[k, 1], e[k, 2]) for k in perm) + " ".join(map(str, order)) + "\n"
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    flags = np.zeros(len(e), np.uint8)
    flags[perm] = np.frombuffer(lines[0].encode(), np.uint8) - 48
    return flags, [int(x) for x in lines[1].split()], [int(x) for x in lines[2].split()], [int(x) for x in lines[3].split()]


def check(emu, e, order, L, B, rec, flags_key, left_key, want):
    perm = np.random.default_rng(len(e)).permutation(len(e))
    flags, (n_in, n_out, n_asym, n_invalid, n_nodes, n_iso), (c_in, r_in, c_out, r_out), left = run_emu(emu, e, order, L, B, perm)
    assert np.array_equal(flags, ru.unpack_flags(rec[flags_key], len(e)))
    assert left == rec[left_key]
    assert (n_in, n_out, n_asym, n_invalid, n_nodes, n_iso, c_in, c_out) == \
           (want["n_in_tip_edges"], want["n_out_tip_edges"], want["n_asymmetric"], 0, want["n_nodes"], want["n_isolated_nodes"],
            want["n_candidates_in"], want["n_candidates_out"])
    assert (r_in > 0) == (c_in > 0) and (r_out > 0) == (c_out > 0)
    return e[flags == 0], left


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    for r in c["results"]:
        e = input_edges(c, r)
        kept, left = check(emu, e, c["order"], r["L"], r["B"], r, "flags", "order_left", r)
        if "second" in r:
            check(emu, kept, left, r["second"]["L"], r["second"]["B"], r, "flags2", "order_left2", r["second"])
