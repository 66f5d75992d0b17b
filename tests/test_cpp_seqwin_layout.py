"""The LDS carve-up of the dependency window's workers (nimfm_amd/csrc/seqwin_layout.h) is plain C++: tests/cpp/seqwin_layout_test.cpp
builds with g++ alone -- no HIP, no library -- and holds its byte counts against the formulas the host used to restate by hand, and
its arrays against overlap, overrun and misalignment (the header against the host's earlier counts and against itself: the
kernels that still carve their LDS by hand are not seen by it).  Built the way tests/test_cpp_csc.py builds its program, without the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_seqwin_layout_test")


def test_seqwin_layout():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "seqwin_layout_test.cpp"), "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seqwin layout ok" in out.stdout
