"""The build of a stage's kernels for the HOST (tools/<stage>_host_emu.cpp), shared by tests/test_<stage>_host_emulation.py.
The sanitizers are what makes those tests worth having, so their flags stand here once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_FLAGS = ("-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def build_emu(tmp_path_factory, stage):
    """Compile tools/<stage>_host_emu.cpp with AddressSanitizer + UBSan and return the program's path."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("emu") / ("%s_host_emu" % stage))
    subprocess.check_call([cxx, *EMU_FLAGS, "-o", exe, os.path.join(ROOT, "tools", "%s_host_emu.cpp" % stage)])
    return exe


def emu_fixture(stage):
    """A module-scoped fixture that builds the stage's emulator once: emu = emu_utils.emu_fixture("contigs")."""
    @pytest.fixture(scope="module")
    def emu(tmp_path_factory):
        return build_emu(tmp_path_factory, stage)
    return emu
