"""Compile-time guard on the kernels of po_layout_coverage (phasm_amd/csrc/coverage.hip.h), by the method of
tests/test_merge_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  Every kernel here is bound by the latency of dependent gathers,
# which only resident waves hide: a row's read, that read's node, the probe sequence of the pair table (k_cov_insert); a
# slot's node, that node's offset (k_cov_fill); an edge's two nodes, their lists, each entry's probe sequence and that
# read's length (k_cov_edges); the binary search of k_cov_members.  k_cov_mark, _nodes and _max stream and need few.
KERNELS = ("k_cov_mark", "k_cov_nodes", "k_cov_members", "k_cov_insert", "k_cov_max", "k_cov_fill", "k_cov_edges")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_coverage_kernels_stay_in_registers(tmp_path):
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
    cov = {k for k in usage if "k_cov_" in k}
    assert len(cov) == len(KERNELS), sorted(cov)           # every k_cov_* kernel is on the list
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found in the compiler remarks" % frag
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
