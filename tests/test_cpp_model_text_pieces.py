"""The decisions of nfm_parse_f64 that are not arithmetic -- tokens, cuts, the carry across a cut, what is clean
(nimfm_amd/csrc/model_text_pieces.h) -- are plain C++: tests/cpp/model_text_pieces_test.cpp builds with g++ alone, reads
texts on stdin and prints what the header's serial walk makes of them.  Held here against float() on every token
(tests/model_text_cases.py).  A second build with -fsanitize=address,undefined runs the same cases stand-alone."""
import functools
import os
import subprocess

import numpy as np
import pytest

import model_text_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "model_text_pieces_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_model_text_pieces_test")


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def run(jobs, sanitize=False):
    """jobs: (text, n_rows, row_len, first_chunk, chunk) -> [(clean, consumed, pieces, fixes, values bytes or None)]"""
    feed = b"".join(b"%d %d %d %d %d\n" % (nr, rl, fc, ch, len(t)) + t for t, nr, rl, fc, ch in jobs)
    out = subprocess.run([exe(sanitize)], input=feed, stdout=subprocess.PIPE, check=True).stdout.split(b"\n")
    res, i = [], 0
    for _ in jobs:
        clean, consumed, pieces, fixes = (int(v) for v in out[i].split())
        i += 1
        vals = None
        if clean:
            vals = np.frombuffer(bytes.fromhex(out[i].decode()), dtype=">u8").astype("<u8").tobytes()
            i += 1
        res.append((bool(clean), consumed, pieces, fixes, vals))
    return res


def all_jobs():
    jobs = []
    for name, (t, nr, rl) in list(MC.clean_cases().items()) + list(MC.not_clean_cases().items()):
        for chunk in (0, 7, 64):
            jobs.append((name, t, nr, rl, 0, chunk))
    t = MC.BLOCK_3x40
    for first in range(2, len(t) + 2):  # a first piece of every length: every legal cut of the block, one at a time
        jobs.append(("cut_%d" % first, t, 3, 40, first, 0))
    for chunk in range(32, 97):
        jobs.append(("chunk_%d" % chunk, t, 3, 40, 0, chunk))
    return jobs


def cuts(t, n_rows, first_chunk, chunk):
    """the restatement of the cuts: -> the ends of the pieces, or None where a token does not fit a piece or lines are missing"""
    def size(c):
        return (128 << 20) if c <= 0 else min(max(c, 2), 1 << 30)
    pos, rows, ends = 0, 0, []
    while True:
        ch = size(first_chunk) if (first_chunk > 0 and not ends) else size(chunk)
        e = len(t) if len(t) - pos <= ch else pos + ch
        nl = [i for i in range(pos, e) if t[i:i + 1] == b"\n"]
        if rows + len(nl) >= n_rows:
            return ends + [nl[n_rows - rows - 1] + 1]
        if e == len(t):
            return ends + [e] if rows + len(nl) == n_rows - 1 and t and not t.endswith(b"\n") else None
        while e > pos and t[e - 1:e] not in (b" ", b"\n"):
            e -= 1
        if e == pos:
            return None
        rows += t.count(b"\n", pos, e)
        ends.append(e)
        pos = e


def check(jobs, results):
    first_cuts = set()
    for (name, t, nr, rl, fc, ch), (clean, consumed, pieces, fixes, vals) in zip(jobs, results):
        want_clean, want_consumed, want_vals = MC.expect(t, nr, rl)
        ends = cuts(t, nr, fc, ch) if nr else []
        want_clean = want_clean and ends is not None  # a token longer than a piece is left to the caller
        assert clean == want_clean, (name, fc, ch)
        if clean:
            assert consumed == want_consumed, (name, fc, ch)
            assert vals == want_vals, (name, fc, ch)
            assert pieces == len(ends), (name, fc, ch)
            if name.startswith("cut_") and pieces > 1:
                first_cuts.add(ends[0])
    return first_cuts


def test_walk_against_float():
    jobs = all_jobs()
    first_cuts = check(jobs, run([j[1:] for j in jobs]))
    # every position after a separator of the 3 x 40 block (but its end) was a cut once
    t = MC.BLOCK_3x40
    assert first_cuts == {i + 1 for i, c in enumerate(t[:-1]) if c in b" \n"}


def test_long_tokens_go_to_strtod():
    t, nr, rl = MC.clean_cases()["tokens_one_row"]
    (clean, _, _, fixes, vals), = run([(t, nr, rl, 0, 0)])
    assert clean and vals == MC.expect(t, nr, rl)[2]
    assert fixes >= 1  # "1.000...031251": more than 19 digits and the cut matters


def test_walk_sanitized():
    jobs = all_jobs()
    check(jobs, run([j[1:] for j in jobs], sanitize=True))


@pytest.mark.parametrize("chunk,want", [(0, 128 << 20), (-3, 128 << 20), (1, 2), (5, 5), (1 << 40, 1 << 30)])
def test_chunk_of(chunk, want):
    # the first piece of a text without separators tells the chunk in force: it cannot be cut, unless it fits
    t = b"1" * 8
    (clean, consumed, pieces, _, _), = run([(t, 1, 1, 0, chunk)])
    assert clean == (want >= len(t))
