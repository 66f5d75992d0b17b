"""crossDecisionFunction and recommend of the C++ host mirror (nimfm_amd/host/nimfm.hpp) build against the
C ABI with plain g++ and, on a GPU, pass tests/cpp/cross_host_test.cpp.  Built the way tests/test_cpp_csc.py builds its test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_cross_host_test")


def _build():
    import __graft_entry__ as g
    g.build()
    lib = os.path.join(ROOT, "nimfm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "cross_host_test.cpp"),
                           "-L", lib, "-lnimfm_hip", "-Wl,-rpath," + lib, "-o", EXE])


def test_cpp_cross_builds():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_cross_runs():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cross host ok" in out.stdout
