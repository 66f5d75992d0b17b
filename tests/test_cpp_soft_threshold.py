"""The device code has one soft threshold (nimfm_amd/csrc/prox_dev.h).  tests/cpp/soft_threshold_test.cpp holds its spelling
against the one cd.hip and pbcd.hip used to carry, bit for bit, over the edge values and two million random pairs: host C++
with -ffp-contract=off, as the library is built.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nimfm_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "soft_threshold_test")
KEPT = ("const double t = fmax(fabs(x) - alpha, 0.0);", "return x > 0 ? t : (x < 0 ? -t : 0.0 * t);")


def test_one_soft_threshold_in_the_device_code():
    """the spelling the C++ test calls `kept` is the header's, and no other file defines a soft threshold"""
    head = open(os.path.join(CSRC, "prox_dev.h")).read()
    body = head[head.index("double soft_threshold(double x, double alpha) {"):]
    body = body[:body.index("}")]
    for line in KEPT:
        assert line in body, line
    test = open(os.path.join(ROOT, "tests", "cpp", "soft_threshold_test.cpp")).read()
    for line in KEPT:
        assert line in test, line
    defs = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, name)).read()
            defs += [(name, m) for m in re.findall(r"double\s+(\w*soft\w*)\s*\(double", text)]
    assert defs == [("prox_dev.h", "soft_threshold")], defs


def test_soft_threshold_spellings_agree():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall",
                           os.path.join(ROOT, "tests", "cpp", "soft_threshold_test.cpp"), "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "soft threshold ok" in out.stdout
