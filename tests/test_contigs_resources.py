"""Compile-time guard on the kernels of po_layout_contigs (phasm_amd/csrc/contigs.hip.h), by the method of
tests/test_superbubbles_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64 VGPRs = 8 waves per SIMD, the most a CDNA SIMD holds.  These kernels gather and are bound by the latency of dependent
# loads, which only resident waves hide: an edge's link and that one's link (k_ct_jump, k_ct_cover_jump), an edge's first
# rank, its in-edge and that one's class (k_ct_links, k_ct_cover_init), an edge's head and the head's words (k_ct_paths,
# k_ct_edge_out).
KERNELS = ("k_ct_init", "k_ct_degrees", "k_ct_classes", "k_ct_links", "k_ct_jump", "k_ct_cover_init", "k_ct_cover_jump", "k_ct_paths",
           "k_ct_filter", "k_ct_isolated", "k_ct_keys", "k_ct_number", "k_ct_iso_table", "k_ct_edge_out")
MAX_VGPRS = 64


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_contig_kernels_stay_in_registers(tmp_path):
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
    mine = {k for k in usage if "k_ct_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)           # every k_ct_* kernel is on the list
    assert not any("k_sb_" in k or "k_scc_" in k or "k_cc_" in k or "k_bc_" in k for k in mine)   # (the tests of those stages count those)
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if re.search(r"\d%sE" % frag, k)}
        assert len(hits) == 1, "kernel %s not found once in the compiler remarks: %s" % (frag, sorted(hits))
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= MAX_VGPRS, "%s uses %d VGPRs (budget %d: 8 waves per SIMD)" % (k, v["VGPRs"], MAX_VGPRS)
