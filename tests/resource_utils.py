"""What hipcc reports about every kernel of the library, compiled once per test process, and the assertions of the
resource guards (tests/test_kernel_resources.py), written once.  hipcc cross-compiles gfx950 without a GPU."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_remarks(text):
    """{mangled kernel name: {"VGPRs": int, "ScratchSize": int, "LDS": int}} of a -Rpass-analysis=kernel-resource-usage stream."""
    usage, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


@functools.lru_cache(maxsize=None)
def _compile():
    """(return code, stderr) of the one compile of the whole library.  Never kept on disk: a stale answer that hides a
    register regression would be worse than the compile's time."""
    src = os.path.join(ROOT, "phasm_amd", "csrc", "c_api.hip")
    with tempfile.TemporaryDirectory() as tmp:
        try:
            out = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-c", src, "-o",
                                  os.path.join(tmp, "c_api.o"), "-Rpass-analysis=kernel-resource-usage"],
                                 capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:      # (kept, like any other outcome: twelve tests do not wait twelve times)
            return -1, "hipcc did not finish within 600 s"
    return out.returncode, out.stderr


@functools.lru_cache(maxsize=None)
def kernel_usage():
    """The resources of every kernel of the library; skips the calling test where there is no hipcc."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    code, err = _compile()
    assert code == 0, err[-2000:]
    return parse_remarks(err)


def check_kernels(usage, spec):
    """Hold the kernels of one stage to its entry of the table.  spec has
      "kernels": {name: (max VGPRs or None, why)} -- every one must be in the remarks and use no scratch;
      "exact":   True: the name is a whole function name of the library's namespace (\\d<name>E) and matches exactly one
                 kernel.  False: the name is the prefix of template instantiations, matches as a substring, at least once;
      "family":  a prefix (or None): the remarks hold as many kernels with it as the list does, and each one is listed,
                 so a new kernel of the stage cannot stay outside the guard;
      "forbid":  prefixes of other families that no member of the family may carry (one kernel, two tables);
      "lds":     {name: most bytes of static LDS per block};
      "why":     what bounds the stage's kernels, and so its budget: said when one goes over."""
    lds = spec.get("lds", {})
    assert set(lds) <= set(spec["kernels"]), sorted(set(lds) - set(spec["kernels"]))
    listed = set()
    for frag, (max_vgpr, why) in spec["kernels"].items():
        if spec["exact"]:
            hits = {k: v for k, v in usage.items() if re.search(r"\d%sE" % frag, k)}
            assert len(hits) == 1, "kernel %s not found once in the compiler remarks: %s" % (frag, sorted(hits))
        else:
            hits = {k: v for k, v in usage.items() if frag in k}
            assert hits, "kernel %s not found in the compiler remarks" % frag
        listed.update(hits)
        for k, v in hits.items():
            assert v["ScratchSize"] == 0, "%s spills to scratch (%d bytes/lane)" % (k, v["ScratchSize"])
            if max_vgpr is not None:
                assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d: %s)\n%s" % (k, v["VGPRs"], max_vgpr, why,
                                                                                         spec.get("why", ""))
            if frag in lds:
                assert v["LDS"] <= lds[frag], "%s holds %d bytes of static LDS (limit %d)" % (k, v["LDS"], lds[frag])
    family = spec.get("family")
    if family:
        mine = {k for k in usage if family in k}
        assert mine <= listed, "%s* kernels that are not on the list: %s" % (family, sorted(mine - listed))
        assert len(mine) == sum(family in frag for frag in spec["kernels"]), sorted(mine)
        for other in spec.get("forbid", ()):
            both = sorted(k for k in mine if other in k)
            assert not both, "%s* kernels that the %s* list counts too: %s" % (family, other, both)
