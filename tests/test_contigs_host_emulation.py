"""The kernels of po_layout_contigs compiled for the HOST (tools/contigs_host_emu.cpp: one lane per wave, threads one after
another) against the goldens, with AddressSanitizer + UBSan: behind the ranks, the degrees and the one in-edge, the class of
every edge, the ranking rounds between two buffer triples, the coverage rounds between two buffer pairs, the sums at the
heads, the filter, the sort of the surviving heads, the table and the two arrays, with the host's caps and batches
(round_phase of components.hip.h, which the library launches by), checked without a GPU.  The edges go in scrambled.  Every
loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import contig_utils as ct
import emu_utils
from test_contigs_oracle import CASES, check_reference, exclude_of, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]
NO_NODE = 0xFFFFFFFF


emu = emu_utils.emu_fixture("contigs")


def run_emu(emu, edges, order, n_total, n_ids, lengths, exclude, min_len):
    X = set(exclude)
    text = "%d %d %d\n" % (n_total, len(edges), len(order)) + "".join("%d %d %d\n" % tuple(e[:3]) for e in edges) + \
           " ".join(map(str, order)) + "\n" + " ".join(str(lengths[n]) for n in order) + "\n" + \
           " ".join(str(int(n in X)) for n in order) + "\n"
    out = subprocess.run([emu, str(min_len), str(n_ids)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_golden(emu, name):
    c = next(x for x in CASES if x["name"] == name)
    stages = stage_inputs(c)
    ints = lambda s: [int(x) for x in s.split()]   # noqa: E731
    node = lambda s: np.asarray([ct.NONE if x == NO_NODE else x for x in ints(s)], np.int64)   # noqa: E731
    for r in c["results"]:
        edges, order, n_ids, lengths = stages[r["stage"]]
        exclude, min_len = exclude_of(c, r), r["min_contig_len"]
        n_total = max([n_ids] + [int(n) + 1 for n in order])   # (merged nodes lie behind the reads)
        perm = np.random.default_rng(len(edges)).permutation(len(edges))
        given = edges[perm] if len(edges) else edges
        lines = run_emu(emu, given.tolist(), order, n_total, n_ids, lengths, exclude, min_len)
        assert len(lines) >= 5, lines[:1]
        n_order, n_excl, n_root, n_late, n_blocked, n_cov, n_uncov, n_paths, n_short, n_iso, n_short_iso, n_contigs, max_nodes = ints(lines[0])
        path_rounds, cover_rounds, batches, max_batch = ints(lines[1])
        table = np.asarray([ints(x) for x in lines[4].split(";") if x.strip()], dtype=np.int64).reshape(-1, 5)
        res = {"edge_contig": node(lines[2]), "edge_pos": node(lines[3]), "c_first": table[:, 0], "c_last": table[:, 1],
               "c_nodes": table[:, 2], "c_first_edge": np.where(table[:, 3] == NO_NODE, ct.NONE, table[:, 3]), "c_length": table[:, 4],
               "stats": {"n_nodes": n_order, "n_edges": len(edges), "n_excluded": n_excl, "n_root_starts": n_root, "n_late_starts": n_late,
                         "n_blocked": n_blocked, "n_covered_edges": n_cov, "n_uncovered_edges": n_uncov, "n_paths": n_paths,
                         "n_short_paths": n_short, "n_isolated": n_iso, "n_short_isolated": n_short_iso, "n_contigs": n_contigs,
                         "max_path_nodes": max_nodes}}
        ct.check_against_record(res, r, given)                                       # the golden
        check_reference(res, given, r)                                               # the reference's paths
        want = ct.scheme(given, order, lengths, exclude, min_len)                    # the restatement, on the edges as given
        for k in ct.ARRAY_KEYS:
            assert np.array_equal(res[k], want[k]), k
        if n_order == 0:
            continue
        # the caps and the batch arithmetic: a batch holds at most 8 rounds, every loop ends within the batch of its closing
        # round; both loops read one set of buffers and write the other, so they need exactly the rounds of the synchronous
        # scheme, which stay within the logarithmic bounds
        assert max_batch <= 8
        path_bound, cover_bound = ct.round_bounds(want["stats"])
        assert path_rounds == r["n_path_rounds"] <= path_bound and cover_rounds == r["n_cover_rounds"] <= cover_bound
        assert (path_rounds > 0) == (cover_rounds > 0) == (len(edges) > 0)
        rounds = path_rounds + cover_rounds
        assert -(-rounds // 8) <= batches <= rounds // 8 + 2      # (at most one part-filled batch per loop)


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    out = subprocess.run([emu, "0"], input="8 3 2\n0 2 1\n2 4 1\n6 0 1\n0 2\n5 5\n0 0\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split("\n")[0] == "invalid 2"
