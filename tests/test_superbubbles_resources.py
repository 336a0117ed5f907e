"""Compile-time guard on the kernels of po_layout_superbubbles (phasm_amd/csrc/superbubbles.hip.h), by the method of
tests/test_partition_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  These kernels stream or gather and are bound by the latency of
# dependent loads, which only resident waves hide: an edge's two ranks and their level words (k_sb_level), a rank's list
# and, per neighbour, the two chains of the tree (k_sb_tree), a rank's dominator and that one's exit (k_sb_encl, k_sb_label).
KERNELS = ("k_sb_init", "k_sb_degrees", "k_sb_fill", "k_sb_nodes", "k_sb_level", "k_sb_level_max", "k_sb_tree", "k_sb_pairs",
           "k_sb_encl", "k_sb_dead_init", "k_sb_dead_round", "k_sb_label", "k_sb_sum", "k_sb_table")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_superbubble_kernels_stay_in_registers(tmp_path):
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
    mine = {k for k in usage if "k_sb_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)           # every k_sb_* kernel is on the list
    assert not any("k_scc_" in k or "k_cc_" in k for k in mine)   # (the partition and components tests count those)
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if re.search(r"\d%sE" % frag, k)}
        assert len(hits) == 1, "kernel %s not found once in the compiler remarks: %s" % (frag, sorted(hits))
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
