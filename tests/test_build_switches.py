"""The switches of the build and of the loader, proven on the host: PHASM_SKIP_ISA_CHECK and PHASM_ALLOW_UNVALIDATED_HIPCC
(phasm_amd/build.py build_library), PHASM_HIP_RUNTIME (phasm_amd/_lib.py _preload_torch_hip_runtime)."""
import os
import re
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_build(monkeypatch, tmp_path, version):
    """phasm_amd.build.build_library with the compiler, the ISA check and the compiler version replaced: what ran."""
    from phasm_amd import build
    ran = []
    lib = str(tmp_path / "libfake.so")

    def check_call(cmd, **kw):
        ran.append("hipcc")
        open(lib, "w").close()

    monkeypatch.setattr(build, "LIB", lib)
    monkeypatch.setattr(build, "subprocess", types.SimpleNamespace(check_call=check_call, CalledProcessError=subprocess.CalledProcessError))
    monkeypatch.setattr(build, "check_scan_isa", lambda: ran.append("isa check"))
    monkeypatch.setattr(build, "hipcc_version", lambda hipcc=None: ran.append("version check") or version)
    return build, lib, ran


def test_build_gate_switches(monkeypatch, tmp_path):
    """PHASM_SKIP_ISA_CHECK skips the post-build ISA and compiler-version checks; PHASM_ALLOW_UNVALIDATED_HIPCC lets a
    compiler the project has not validated through.  Without either, such a compiler's library is removed."""
    for k in ("PHASM_SKIP_ISA_CHECK", "PHASM_ALLOW_UNVALIDATED_HIPCC"):
        monkeypatch.delenv(k, raising=False)
    build, lib, ran = _fake_build(monkeypatch, tmp_path, "0.0-unvalidated")
    with pytest.raises(RuntimeError, match="not one of"):
        build.build_library(force=True)
    assert ran == ["hipcc", "isa check", "version check"] and not os.path.exists(lib)
    monkeypatch.setenv("PHASM_ALLOW_UNVALIDATED_HIPCC", "1")
    ran.clear()
    assert build.build_library(force=True) == lib and os.path.exists(lib)
    assert ran == ["hipcc", "isa check", "version check"]
    monkeypatch.delenv("PHASM_ALLOW_UNVALIDATED_HIPCC")
    monkeypatch.setenv("PHASM_SKIP_ISA_CHECK", "1")
    ran.clear()
    assert build.build_library(force=True) == lib and os.path.exists(lib)
    assert ran == ["hipcc"]


_RUNTIME_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from phasm_amd import _lib
_lib._preload_torch_hip_runtime()
with open("/proc/self/maps") as f:
    maps = [l.split()[-1] for l in f if "libamdhip64" in l]
print("TORCH_RUNTIME %%d" %% any("/torch/lib/" in p for p in maps))
"""


def test_hip_runtime_switch_skips_the_torch_preload():
    """phasm_amd/_lib.py maps torch's bundled libamdhip64 before the library (one HIP runtime per process);
    PHASM_HIP_RUNTIME=system leaves the choice to the dynamic loader.  Children started by the checker process."""
    import importlib.util
    import checker as ck
    spec = importlib.util.find_spec("torch")
    assert spec is not None and spec.submodule_search_locations
    assert os.path.exists(os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so"))
    out = {}
    for value in (None, "system"):
        env = {k: v for k, v in os.environ.items() if k != "PHASM_HIP_RUNTIME"}
        if value:
            env["PHASM_HIP_RUNTIME"] = value
        rc, stdout, stderr = ck.run([sys.executable, "-c", _RUNTIME_CHILD % {"root": ROOT}], env=env, capture_output=True,
                                    text=True, timeout=120)
        assert rc == 0 and "TORCH_RUNTIME" in stdout, stdout[-2000:] + stderr[-2000:]
        out[value] = int(re.search(r"TORCH_RUNTIME (\d)", stdout).group(1))
    assert out == {None: 1, "system": 0}, out
