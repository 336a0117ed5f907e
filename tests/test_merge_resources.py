"""Compile-time guard on the kernels of po_layout_merge (phasm_amd/csrc/merge.hip.h), by the method of
tests/test_diamond_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds: every kernel here is bound by the latency of dependent
# gathers (a node's one edge, that edge's other end, that node's degree; jb[jb[n]] in a round), which only resident
# waves hide.
KERNELS = ("k_merge_degree", "k_merge_links", "k_merge_jump", "k_merge_tails", "k_merge_bitonic", "k_merge_number", "k_merge_tables",
           "k_merge_ranks", "k_merge_edges")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_merge_kernels_stay_in_registers(tmp_path):
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
    merge = {k for k in usage if "k_merge_" in k}
    assert len(merge) == len(KERNELS), sorted(merge)       # every k_merge_* kernel is on the list
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found in the compiler remarks" % frag
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
