"""Compile-time guard on the kernels of po_layout_reduce (phasm_amd/csrc/reduce.hip.h), by the method of
tests/test_kernel_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (max VGPRs, why).  64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds: every kernel here is bound by
# the latency of dependent gathers (an edge, then its node's lists), which only resident waves hide.  k_reduce_mark
# runs one 64-lane workgroup per node with 5 KB of LDS: 32 of them fit a CU's 160 KB, so registers, not LDS, must not
# be what limits its occupancy either.
BUDGET = {
    "k_reduce_degree": (64, "8 waves per SIMD"),
    "k_reduce_maxdeg": (64, "same"),
    "k_reduce_scatter": (64, "same"),
    "k_reduce_order": (64, "same"),
    "k_reduce_mark": (64, "same; LDS allows 32 workgroups of one wave per CU"),
    "k_reduce_symmetric": (64, "same"),
    "k_reduce_emit": (64, "same"),
}
MARK_LDS_MAX = 160 * 1024 // 32


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_reduce_kernels_stay_in_registers(tmp_path):
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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for frag, (max_vgpr, why) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found in the compiler remarks" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d: %s)" % (k, v["VGPRs"], max_vgpr, why)
    mark = [v for k, v in usage.items() if "k_reduce_mark" in k]
    assert all(v["LDS"] <= MARK_LDS_MAX for v in mark), mark
