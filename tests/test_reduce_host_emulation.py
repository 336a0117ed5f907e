"""The kernels of po_layout_reduce compiled for the HOST (tools/reduce_host_emu.cpp: one lane per wave, threads one
after another) against the reference's goldens, with AddressSanitizer + UBSan: indexing and logic of the CSR build,
of k_reduce_mark with its states in "LDS" and in the global workspace (the hubs, on both sides of the switch at 1024 out-edges), and of the symmetry pass, checked
without a GPU.  The edges go in shuffled with their insertion rank beside them, as the table path hands them over."""
import subprocess

import numpy as np
import pytest

import emu_utils
import layout_utils as lu
import reduce_utils as ru
from oracle import layout_oracle as lo
from phasm_amd.io import gfa

NAMES = ["ladder_varlen", "ladder_cfg2_mini", "layout_random_1008", "layout_daligner_form_2003", "line_100", "line_105",
         "line_111", "hub_5200", "hub_1023", "hub_1024", "hub_1025", "stagger_1100", "dense_260", "tie_8"]


emu = emu_utils.emu_fixture("reduce")


GOLDEN = ru.load_golden()


def stage1(c):
    names, lengths, rows = gfa.read_gfa2_rows(ru.case_text(c).splitlines(True))
    got = lo.layout_sequential(rows, lu.node_lengths(lengths), **c["params"])["edges"]
    s1 = np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4)
    assert len(s1) == c["n_stage1"] > 0
    return names, s1


def run_emu(emu, n_nodes, fuzz, edges, rank, perm):
    """Flags per edge (in the order of ``edges``) and the counters, the edges handed over in the order ``perm``."""
    text = "%d %s %d\n" % (n_nodes, fuzz, len(edges)) + "".join("%d %d %d %d\n" % (edges[k, 0], edges[k, 1], edges[k, 2], rank[k]) for k in perm)
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    flags = np.zeros(len(edges), np.uint8)
    flags[perm] = np.frombuffer(lines[0].encode(), np.uint8) - 48
    return flags, [int(x) for x in lines[1].split()]


SECOND = GOLDEN["second_pass"]


@pytest.mark.parametrize("rec", SECOND, ids=["%s-F%d-F%d" % (r["case"], r["fuzz"], r["fuzz2"]) for r in SECOND])
def test_host_compiled_kernels_on_a_kept_result(emu, rec):
    """A second pass: the kept edges of the first with the rank they had there, which is no permutation of 0..n-1."""
    c = next(x for x in GOLDEN["cases"] if x["name"] == rec["case"])
    names, s1 = stage1(c)
    keep = np.flatnonzero(ru.unpack_flags(c["results"][str(rec["fuzz"])]["flags_by_uv"], len(s1))[np.argsort(np.lexsort((s1[:, 1], s1[:, 0])))] == 0)
    kept = s1[keep]
    assert len(kept) == rec["n_in"]
    flags, (n_trans, n_asym, _, n_invalid) = run_emu(emu, 2 * len(names), rec["fuzz2"], kept, keep, np.random.default_rng(2).permutation(len(kept)))
    assert np.array_equal(flags[np.lexsort((kept[:, 1], kept[:, 0]))], ru.unpack_flags(rec["flags_by_uv"], len(kept)))
    assert (n_trans, n_asym, n_invalid) == (rec["n_transitive"], rec["n_asymmetric"], 0)


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in GOLDEN["cases"] if x["name"] == name)
    names, s1 = stage1(c)
    perm = np.random.default_rng(1).permutation(len(s1))
    order = np.lexsort((s1[:, 1], s1[:, 0]))
    for fuzz, exp in c["results"].items():
        flags, (n_trans, n_asym, max_deg, n_invalid) = run_emu(emu, 2 * len(names), fuzz, s1, np.arange(len(s1)), perm)
        assert np.array_equal(flags[order], ru.unpack_flags(exp["flags_by_uv"], len(s1))), fuzz
        assert (n_trans, n_asym, n_invalid) == (exp["n_transitive"], exp["n_asymmetric"], 0)
        assert max_deg == int(np.bincount(s1[:, 0]).max())
