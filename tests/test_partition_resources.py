"""Compile-time guard on the kernels of po_layout_partition (phasm_amd/csrc/partition.hip.h), by the method of
tests/test_components_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  These kernels stream or gather and are bound by the latency of
# dependent loads, which only resident waves hide: an edge's two ranks, their live bytes and their colour words or mark
# bytes (k_scc_trim_edges, k_scc_forward, k_scc_backward), an edge's two SCCs and their table entries (k_scc_edges), a rank's
# root and that root's index (k_scc_label_nodes).
KERNELS = ("k_scc_init", "k_scc_trim_edges", "k_scc_trim_ranks", "k_scc_colour_init", "k_scc_forward", "k_scc_back_init",
           "k_scc_backward", "k_scc_retire", "k_scc_roots", "k_scc_label_nodes", "k_scc_edges", "k_scc_flags", "k_scc_max")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_partition_kernels_stay_in_registers(tmp_path):
    src = os.path.join(ROOT, "phasm_amd", "csrc", "c_api.hip")
    out = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-c", src, "-o",
                          str(tmp_path / "c_api.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    mine = {k for k in usage if "k_scc_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)           # every k_scc_* kernel is on the list
    assert not any("k_cc_" in k for k in mine)               # (tests/test_components_resources.py counts those)
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found in the compiler remarks" % frag
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
