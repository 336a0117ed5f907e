"""Compile-time guard on the kernels of po_layout_components (phasm_amd/csrc/components.hip.h), by the method of
tests/test_coverage_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  These kernels stream or gather and are bound by the latency of
# dependent loads, which only resident waves hide: an edge's two ranks and their parent words (k_cc_hook), a rank's parent
# and grandparent (k_cc_jump), a rank's root and that root's index (k_cc_label_nodes).
KERNELS = ("k_cc_keys", "k_cc_init", "k_cc_ends", "k_cc_hook", "k_cc_jump", "k_cc_roots", "k_cc_label_nodes", "k_cc_label_edges",
           "k_cc_max")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_components_kernels_stay_in_registers(tmp_path):
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
    mine = {k for k in usage if "k_cc_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)           # every k_cc_* kernel is on the list
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found in the compiler remarks" % frag
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
