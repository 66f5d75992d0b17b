"""The dataset ops of the C++ host mirror (nimfm_amd/host/nimfm.hpp) build against the C ABI with plain g++ and, on a GPU, pass
tests/cpp/dataset_ops_host_test.cpp: X[indices], slice, shuffle, vstack, hstack, normalize and loadUserItemRatingFile are the C
ABI's calls, with the reference's error texts.  Built the way tests/test_cpp_psgd.py builds its test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dataset_ops_host_test")


def _build():
    import __graft_entry__ as g
    g.build()
    lib = os.path.join(ROOT, "nimfm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "dataset_ops_host_test.cpp"),
                           "-L", lib, "-lnimfm_hip", "-Wl,-rpath," + lib, "-o", EXE])


def test_cpp_dataset_ops_builds():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_dataset_ops_runs():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dataset ops host ok" in out.stdout
