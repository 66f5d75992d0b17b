"""Host-side check of nimfm_amd/csrc/format_num.h (binary64 -> shortest decimal text, what the dump kernels run on the
GPU, compiled here for the CPU from the same source) against nimfm_amd.host._nim_float, i.e. Python's repr with Nim's
spelling of nan / inf: byte equality of every token, and every token read back by parse_num.h's parse_float to the same
bits.  The program is built a second time with AddressSanitizer and UBSan and run on the same corpus."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "format_num_test.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _nim_float(v):  # nimfm_amd/host.py::_nim_float, restated: importing the package needs the native library
    if v != v:
        return "nan"
    if v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    return repr(v)


def _build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("format_num_test")


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


@pytest.fixture(scope="module")
def corpus():
    rnd = random.Random(24)
    top = 0x7FEFFFFFFFFFFFFF  # DBL_MAX
    b = [0, 1 << 63, 1, (1 << 52) - 1, 1 << 52, top, top | 1 << 63]
    b += [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
          0x7FF4000000000abc, 0x7FF0000000000000, 0xFFF0000000000000]

    def with_neighbours(x):
        c = bits_of(x)
        return [v for v in (c - 1, c, c + 1) if 0 <= v <= top]

    for e in range(-1074, 1024):
        b += with_neighbours(2.0 ** e)
    for q in range(-323, 309):
        b += with_neighbours(float("1e%d" % q))
    for x in (9999999999999998.0, 1e16, 0.0001, 9.999999999999999e-05, 123456.0, 1.0, 9007199254740992.0,
              1.2345678901234568e17, 5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-5, 1e22, 1e23, 0.3):
        b += with_neighbours(abs(x)) + [bits_of(x)]
    ints = list(range(0, 70000)) + [2 ** 53 - 2, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2] + [rnd.randrange(2 ** 53) for _ in range(30000)]
    ints += [10 ** k + o for k in range(1, 16) for o in (-1, 0, 1)]
    b += [bits_of(float(i)) for i in ints]
    b += [rnd.getrandbits(64) for _ in range(1000000)]
    for _ in range(100000):
        k = rnd.randint(1, 17)
        b.append(bits_of(round(rnd.uniform(-1, 1) * 10.0 ** rnd.randint(-3, 6), k)))
    return b


def _run(exe, corpus):
    text = "".join("%x\n" % v for v in corpus)
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def _compare(corpus, out):
    assert len(out) == len(corpus) + 1 and out[-1] == ""
    longest = 0
    for v, o in zip(corpus, out):
        tok, back = o.split(" ")
        x = from_bits(v)
        assert tok == _nim_float(x), (hex(v), tok, _nim_float(x))
        if x != x:
            assert from_bits(int(back, 16)) != from_bits(int(back, 16)), (hex(v), o)
        else:
            assert int(back, 16) == v, (hex(v), o)
        longest = max(longest, len(tok))
    assert longest == 24


def test_format_float_is_repr_and_reads_back(exe, corpus):
    assert len(corpus) > 1100000
    _compare(corpus, _run(exe, corpus))


def test_format_float_under_sanitizers(corpus):
    san = _build("format_num_test_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _compare(corpus, _run(san, corpus))


def test_format_uint(exe):
    vals = [0, 9, 10, 2 ** 31 - 1, 2 ** 32, 2 ** 64 - 1, 99, 100, 12345678901234567890]
    out = subprocess.run([exe, "uint"], input="".join("%d\n" % v for v in vals), capture_output=True, text=True, check=True).stdout
    assert out.split("\n")[:-1] == [str(v) for v in vals]


def test_generated_table_is_current():
    """fmt_pow5_table.h is what tools/gen_fmt_pow5_table.py writes (checked by value, the generator is not run)"""
    import re
    h = open(os.path.join(ROOT, "nimfm_amd", "csrc", "fmt_pow5_table.h")).read()
    rows = [(int(a, 16) << 64) | int(c, 16) for a, c in re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\}", h)]
    assert len(rows) == 292 + 326
    for i in (0, 1, 27, 150, 291):
        p = 5 ** i
        assert rows[i] == (1 << (p.bit_length() - 1 + 125)) // p + 1
    for i in (0, 1, 55, 200, 325):
        p = 5 ** i
        s = p.bit_length() - 125
        assert rows[292 + i] == (p >> s if s >= 0 else p << -s)
