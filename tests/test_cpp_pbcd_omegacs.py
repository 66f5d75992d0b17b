"""PBCD<L, OmegaCS> of the C++ host mirror (nimfm_amd/host/nimfm.hpp) builds against the C ABI with plain g++ and, on a GPU,
passes tests/cpp/pbcd_omegacs_host_test.cpp: at degrees 2 and 3 the class is the C ABI's calls bit for bit, the solvers
without a step for OmegaCS refuse it, and regEval gives what the Python host's eval gives.  Built the way
tests/test_cpp_pbcd.py builds its test."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_pbcd_omegacs_host_test")


def _build():
    import __graft_entry__ as g
    g.build()
    lib = os.path.join(ROOT, "nimfm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "pbcd_omegacs_host_test.cpp"),
                           "-L", lib, "-lnimfm_hip", "-Wl,-rpath," + lib, "-o", EXE])


def test_cpp_pbcd_omegacs_builds():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_pbcd_omegacs_runs():
    import nimfm_amd as nf
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pbcd omegacs host ok" in out.stdout
    Po = np.array([((t * 7) % 11 - 5) / 8.0 for t in range(15)]).reshape(3, 5)  # [k][da], the test program's values
    got = {int(l.split()[1]): float(l.split()[2]) for l in out.stdout.splitlines() if l.startswith("regeval ")}
    assert sorted(got) == [1, 2, 3, 4]
    for degree, value in got.items():
        np.testing.assert_allclose(value, nf.newOmegaCS().eval(Po.T, degree), rtol=1e-14)
