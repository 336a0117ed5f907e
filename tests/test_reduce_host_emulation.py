"""The kernels of po_layout_reduce compiled for the HOST (tools/reduce_host_emu.cpp: one lane per wave, threads one
after another) against the reference's goldens, with AddressSanitizer + UBSan: indexing and logic of the CSR build,
of k_reduce_mark with its states in "LDS" and in the global workspace (the hub), and of the symmetry pass, checked
without a GPU.  The edges go in shuffled with their insertion rank beside them, as the table path hands them over."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import layout_utils as lu
import reduce_utils as ru
from oracle import layout_oracle as lo
from phasm_amd.io import gfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ladder_varlen", "ladder_cfg2_mini", "layout_random_1008", "layout_daligner_form_2003", "line_100", "line_105",
         "line_111", "hub_5200"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("emu") / "reduce_host_emu")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tools", "reduce_host_emu.cpp")])
    return exe


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_kernels_equal_the_reference(emu, name):
    c = next(x for x in ru.load_golden()["cases"] if x["name"] == name)
    names, lengths, rows = gfa.read_gfa2_rows(ru.case_text(c).splitlines(True))
    got = lo.layout_sequential(rows, lu.node_lengths(lengths), **c["params"])["edges"]
    s1 = np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4)
    assert len(s1) == c["n_stage1"] > 0
    perm = np.random.default_rng(1).permutation(len(s1))
    order = np.lexsort((s1[:, 1], s1[:, 0]))
    for fuzz, exp in c["results"].items():
        text = "%d %s %d\n" % (2 * len(names), fuzz, len(s1)) + "".join("%d %d %d %d\n" % (s1[k, 0], s1[k, 1], s1[k, 2], k) for k in perm)
        out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.split("\n")
        flags = np.zeros(len(s1), np.uint8)
        flags[perm] = np.frombuffer(lines[0].encode(), np.uint8) - 48
        assert np.array_equal(flags[order], ru.unpack_flags(exp["flags_by_uv"], len(s1))), fuzz
        n_trans, n_asym, max_deg, n_invalid = (int(x) for x in lines[1].split())
        assert (n_trans, n_asym, n_invalid) == (exp["n_transitive"], exp["n_asymmetric"], 0)
        assert max_deg == int(np.bincount(s1[:, 0]).max())
