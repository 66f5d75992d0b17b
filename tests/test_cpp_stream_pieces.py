"""Where the body of a binary stream file is cut into the pieces the device packs (nimfm_amd/csrc/stream_pieces.h) is plain
C++: tests/cpp/stream_pieces_test.cpp builds with g++ alone -- no HIP, no library -- reads cases on stdin and prints the header's
cuts, which are held here against a plain restatement.  Built the way tests/test_cpp_seq_route.py builds its program; a second
build with -fsanitize=address,undefined runs stand-alone."""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stream_pieces_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_stream_pieces_test")
DEFAULT, CAP = 128 << 20, 1 << 30


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def pieces(counts, esize, chunk_bytes):
    """the restatement: records are taken while the piece stays within the chunk, one at least"""
    chunk = DEFAULT if chunk_bytes <= 0 else min(chunk_bytes, CAP)
    size = [8 + esize * c for c in counts]
    cut, spans, r = [0], [], 0
    while r < len(size):
        b, r1 = size[r], r + 1
        while r1 < len(size) and b + size[r1] <= chunk:
            b += size[r1]
            r1 += 1
        cut.append(r1)
        spans.append(b)
        r = r1
    return chunk, max(spans, default=0), sum(size), cut


def cases():
    rng = np.random.default_rng(7)
    out = []
    for esize in (16, 24):
        short = [0, 1, 2, 3, 1, 0, 2]
        out += [
            ("smaller_than_every_record", esize, 8, [1, 2, 3, 1]),            # every record is a piece by itself
            ("smaller_than_a_count_word", esize, 1, [0, 0, 1]),
            ("equal_to_a_record", esize, 8 + 2 * esize, [2, 2, 0, 2, 1, 1]),
            ("equal_to_two_records", esize, 2 * (8 + esize), [1, 1, 1, 1, 1]),
            ("one_long_among_short", esize, 8 * len(short) + 6 * esize, short + [5000] + short),
            ("all_empty", esize, 24, [0] * 10),
            ("all_empty_one_piece", esize, 0, [0] * 10),
            ("no_records", esize, 24, []),
            ("default_chunk", esize, 0, [3] * 50),
            ("negative_chunk", esize, -5, [3] * 50),
            ("chunk_above_the_cap", esize, 1 << 40, [3] * 50),
            ("one_record", esize, 64, [7]),
        ]
        for i in range(200):
            n = int(rng.integers(1, 40))
            counts = [int(c) for c in rng.integers(0, 9, n)]
            if i % 4 == 0:
                counts[int(rng.integers(0, n))] = int(rng.integers(50, 400))
            out.append(("random%d" % i, esize, int(rng.integers(1, 600)), counts))
    return out


def run(cs, sanitize=False):
    lines = ["%d %d %d %s" % (esize, chunk, len(counts), " ".join(map(str, counts))) for _, esize, chunk, counts in cs]
    out = subprocess.run([exe(sanitize)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(cs) and "%d cases" % len(cs) in out.stderr
    res = []
    for ln in got:
        head, cut = ln.split("|")
        res.append(tuple(int(v) for v in head.split()) + ([int(v) for v in cut.split()],))
    return res


def test_the_cuts_of_every_case_are_the_restatements():
    cs = cases()
    for (name, esize, chunk, counts), got in zip(cs, run(cs)):
        assert got == pieces(counts, esize, chunk), (name, esize, chunk, counts, got)


def test_the_named_cases_cut_where_the_format_says():
    by = {(name, esize): pieces(counts, esize, chunk) for name, esize, chunk, counts in cases()}
    for esize in (16, 24):
        assert by["smaller_than_every_record", esize][3] == [0, 1, 2, 3, 4]
        assert by["equal_to_a_record", esize][3] == [0, 1, 2, 3, 4, 5, 6] and by["equal_to_a_record", esize][1] == 8 + 2 * esize
        assert by["equal_to_two_records", esize][3] == [0, 2, 4, 5]
        cut = by["one_long_among_short", esize][3]
        assert (7, 8) in zip(cut, cut[1:])  # the long record is a piece by itself
        assert by["one_long_among_short", esize][1] == 8 + 5000 * esize
        assert by["all_empty", esize][3] == [0, 3, 6, 9, 10] and by["all_empty_one_piece", esize][3] == [0, 10]
        assert by["no_records", esize][3] == [0] and by["no_records", esize][1:3] == (0, 0)
        assert by["default_chunk", esize][0] == by["negative_chunk", esize][0] == DEFAULT and by["chunk_above_the_cap", esize][0] == CAP


def test_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined: no report (a report ends it with a nonzero status), the same answers"""
    cs = cases()
    assert run(cs, sanitize=True) == run(cs)


def test_the_packer_cuts_by_the_header():
    with open(os.path.join(ROOT, "nimfm_amd", "csrc", "dataset_stream.hip")) as f:
        text = f.read()
    assert '#include "stream_pieces.h"' in text and text.count("stream_pieces(") == 1
    with open(os.path.join(ROOT, "nimfm_amd", "csrc", "stream_pieces.h")) as f:
        head = f.read()
    assert "#include <hip" not in head and '"common.h"' not in head
