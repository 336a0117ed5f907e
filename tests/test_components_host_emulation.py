"""The kernels of po_layout_components compiled for the HOST (tools/components_host_emu.cpp: one lane per wave, threads one
after another) against the goldens, with AddressSanitizer + UBSan: the sort of the rank words, the ranks of the edge ends,
the hook and jump rounds with the host's cap and batches, the numbering of the roots, the labels and the table, checked
without a GPU.  The edges go in scrambled.  Every loop is bounded: a subprocess that runs into its timeout fails the test."""
import subprocess

import numpy as np
import pytest

import components_utils as cu
import emu_utils
from test_components_oracle import CASES, stage_inputs

NAMES = [c["name"] for c in CASES if c.get("direct")] + \
        ["tangle_3", "selfish_2", "reduced_hub_1025", "reduced_line_101", "ring_40", "lasso_70_6"] + \
        [c["name"] for c in CASES if c["name"].startswith("union_")]


emu = emu_utils.emu_fixture("components")


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
        assert len(lines) >= 4, lines[:1]
        n_order, n_comp, n_single, max_n, max_e, rounds, batches, cap = ints(lines[0])
        edge_comp = np.zeros(len(uv), np.int64)
        edge_comp[perm] = ints(lines[2])
        table = np.asarray([ints(x) for x in lines[3].split(";") if x], dtype=np.int64).reshape(-1, 3)
        res = {"node_component": ints(lines[1]), "edge_component": edge_comp, "first_node": table[:, 0], "n_nodes": table[:, 1],
               "n_edges": table[:, 2],
               "stats": {"n_nodes": n_order, "n_edges": len(uv), "n_components": n_comp, "n_singletons": n_single,
                         "max_component_nodes": max_n, "max_component_edges": max_e}}
        cu.check_against_record(res, r)
        assert edge_comp.tolist() == cu.weak_components(uv, order)["edge_component"].tolist()
        assert cap == n_order + 2 and rounds <= cap and batches == -(-rounds // 8) and (rounds > 0) == (n_order > 0)
        if name.startswith("direct_path_4097_"):
            # hooking alone is linear in the diameter (4 096 here); with the jumps the synchronous scheme takes 13 rounds
            assert 8 * rounds <= n_order


def test_an_edge_end_outside_the_node_order_is_counted(emu):
    assert run_emu(emu, [(0, 2), (2, 4), (6, 0)], [0, 2], 8, [0, 1, 2])[0] == "invalid 2"
