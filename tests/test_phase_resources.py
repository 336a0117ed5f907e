"""Compile-time guard on the kernels of po_phase_branch (phasm_amd/csrc/phase.hip.h), by the method of
tests/test_contigs_resources.py: hipcc cross-compiles gfx950 without a GPU and reports every kernel's resources."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("k_ph_bits", "k_ph_intervals", "k_ph_table", "k_ph_extend", "k_ph_gather", "k_ph_levels", "k_ph_survive")
MAX_LDS = 64 * 1024


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_phase_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
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
    mine = {k for k in usage if "k_ph_" in k}
    assert len(mine) == len(KERNELS), sorted(mine)           # every k_ph_* kernel is on the list
    for frag in KERNELS:
        hits = {k: v for k, v in usage.items() if re.search(r"\d%sE" % frag, k)}
        assert len(hits) == 1, "kernel %s not found once in the compiler remarks: %s" % (frag, sorted(hits))
        for k, v in hits.items():
            print(k, v)
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            assert v["LDS"] <= MAX_LDS, "%s holds %d bytes of static LDS" % (k, v["LDS"])
