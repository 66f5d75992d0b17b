"""CPU: the properties the texts of tests/ingest_edge_cases.py must have so that tests/test_gpu_ingest_edges.py takes
ingest.hip to the edges their names claim -- which byte holds which delimiter, which residues mod 64 they cover, how long
the texts, rows and runs are against a tile, how many lines and entries against one launch -- and the strings of the source
those figures restate.  No GPU.  The oracle must accept every well-formed case; the tokens listed as taking the strtod
fix-up must return flag 1 from the host build of parse_num.h (tests/cpp/parse_num_test, as tests/test_parse_num.py builds it)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import ingest_edge_cases as E
from test_parse_num import HARD, exe, reference  # noqa: F401  (exe: the module-scoped fixture that builds parse_num_test)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")
ALL64 = set(range(64))


def test_the_source_still_has_the_figures_restated():
    src = open(os.path.join(CSRC, "ingest.hip")).read()
    common = open(os.path.join(CSRC, "common.h")).read()
    assert "constexpr int kBlock = 256;" in common
    assert "constexpr int kChunk = 64;" in src and "constexpr int kTile = kBlock * kChunk;" in src
    assert E.TILE == 256 * E.CHUNK
    assert "if (b > 256 * 64) b = 256 * 64;" in src and E.GRID_CAP == 256 * 64 * 256
    assert "constexpr int kMaxFix = 1 << 20;" in src and E.MAX_FIX == 1 << 20
    assert "std::min<int64_t>(n_tiles, 256 * 32)" in src and E.TILE_GRID_CAP == 256 * 32
    assert "text->alloc((size_t)len + 64)" in src and "text.alloc((size_t)len + 64)" in src


def flags_of(exe, tokens):
    out = subprocess.run([exe], input="\n".join(tokens) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res = []
    for t, o in zip(tokens, out):
        c, fl, _ = o.split()
        assert int(c) == len(t), (t, o)  # read whole
        res.append(int(fl))
    return res


def test_delims_at_every_offset():
    cases = E.delims_at_every_offset()
    names = [c[0] for c in cases]
    for fmt in ("svm", "ffm"):
        for what in ("newline", "colon"):
            for at in (E.TILE - 1, E.TILE):
                assert "delims_%s_%s_at_%d" % (fmt, what, at) in names
    for name, text, ffm, _ in cases:
        assert len(text) >= 3 * E.TILE, name
        nl, co = E.positions(text, "\n"), E.positions(text, ":")
        assert set(nl % 64) == ALL64 and set(co % 64) == ALL64, name
        at = int(name.rsplit("_", 1)[1])
        if "entry_across" in name:
            k = int(np.searchsorted(co, E.TILE - 1))
            assert co[k] == E.TILE - 1 and k % 2 == 0, name  # the FIRST colon of its entry is the last byte of tile 0
            entry = text[text.rfind(" ", 0, co[k]) + 1:co[k + 1] + 1]
            assert co[k + 1] >= E.TILE and entry.count(":") == 2 and entry.replace(":", "").isdigit(), (name, entry)
        else:
            assert text[at] == ("\n" if "newline" in name else ":"), name
        r = E.expect(text, ffm)
        assert len(r["y"]) == len(nl) and len(r["data"]) == len(co) // (2 if ffm else 1), name


@functools.lru_cache(maxsize=None)
def counts_of(head):
    r = E.expect(head, False) if head else {"y": [], "data": []}
    return len(r["y"]), len(r["data"])


def test_length_sweep():
    cases = E.length_sweep()
    by = {c[0]: c[1] for c in cases}
    for length in E.SWEEP_LENGTHS:
        for ending in E.ENDINGS:
            text = by.get("length_%d_%s" % (length, ending))
            if text is None:
                assert ending == "colon_at_len_minus_2" and length < 5, (length, ending)  # "<t> 5:7" needs five bytes
                continue
            assert len(text) == length == len(text.encode())
            if ending == "newline":
                assert text[-1] == "\n"
            elif ending == "no_newline":
                assert text[-1].isdigit()
            else:
                assert text[-2] == ":" and text[-1].isdigit() and text.rfind(":") == length - 2
            # the oracle accepts it: the whole lines the long texts share once, what follows them per text
            cut = text.rfind("\n", 0, max(0, length - 200)) + 1
            lines, entries = counts_of(text[:cut])
            r = E.expect(text[cut:], False)
            assert lines + len(r["y"]) == text.count("\n") + (text[-1] != "\n") and entries + len(r["data"]) == text.count(":")
    assert len(cases) == 3 * len(E.SWEEP_LENGTHS) - 4
    assert set(range(E.TILE - 72, E.TILE + 73)) <= set(E.SWEEP_LENGTHS) and set(range(1, 81)) <= set(E.SWEEP_LENGTHS)
    # every end position inside a 64-byte chunk, an 8-byte word and a 16-byte load, on both sides of the tile edge
    assert {n % 64 for n in E.SWEEP_LENGTHS if n > 80} == ALL64 and {n % 64 for n in E.SWEEP_LENGTHS if n <= 80} == ALL64
    d = E.dirt()
    assert len(d) == 1 << 20 and set(d) == {":", "\n"}  # malformed for the device: every line lacks its target


def test_long_rows():
    for name, text, ffm, _ in E.long_rows():
        r = E.expect(text, ffm)
        assert list(np.diff(r["indptr"])) == E.LONG_ROW_LENGTHS, name
        lens = [len(ln) + 1 for ln in text.split("\n")[:-1]]
        assert E.TILE < lens[1] < 4 * E.TILE < lens[5], (name, lens)  # more than one tile, more than four
        assert lens[1] / 3000 < 14 and lens[5] / 9000 < 14
        row = r["indices"][r["indptr"][5]:r["indptr"][6]]
        assert np.any(np.diff(row) < 0) and len(set(row.tolist())) < len(row), name  # unsorted, repeated
        mag = np.abs(r["data"][r["data"] != 0])
        assert mag.min() < 1e-7 and mag.max() > 1e6, name  # the decade spread


def test_empty_runs():
    cases = {c[0]: c[1] for c in E.empty_runs()}
    lf, crlf = cases["empty_runs_lf"], cases["empty_runs_crlf"]
    assert crlf[E.TILE - 1] == "\r" and crlf[E.TILE] == "\n"  # the pair straddles the tile edge
    for text, sep in ((lf, "\n"), (crlf, "\r\n")):
        lines = text.split(sep)
        assert lines[-1] == "" and len(lines) - 1 == 3 + sum(E.EMPTY_RUNS)
        run = [i for i, ln in enumerate(lines[:-1]) if ln]
        assert run == [0, 1 + E.EMPTY_RUNS[0], 2 + E.EMPTY_RUNS[0] + E.EMPTY_RUNS[1]]
        nl = E.positions(text, "\n")
        gap = nl[run[1] + 1:run[2]]  # the newlines of the 20000 empty lines
        assert len(gap) >= E.EMPTY_RUNS[1] - 1 > 256 * 64  # more than the 16384 bytes a workgroup scans
        assert gap[0] // E.TILE < gap[-1] // E.TILE  # across a tile edge
        r = E.expect(text, False)
        y = r["y"]
        assert len(y) == len(lines) - 1 and list(np.diff(r["indptr"])[run]) == [0, 2, 2] and r["indptr"][-1] == 4
        assert np.all(y[:run[1]] == y[0]) and np.all(y[run[1]:run[2]] == -1.0) and np.all(y[run[2]:] == 2.0)


def test_hard_numbers(exe):
    toks = E.hard_number_tokens()
    assert len(toks) >= 20000
    assert [t for t in HARD if reference(t)[0] == len(t) and t] == E.HARD  # the accepted forms of test_parse_num.py's list
    flagged = E.FLAGGED + ["-" + t for t in E.FLAGGED]
    assert flags_of(exe, flagged) == [1] * len(flagged)
    gen = E.generated_tokens()
    # more than 19 digits and NOT flagged: the truncated significand decides on the device.  Only the digit strings can
    # hold such tokens -- repr() of a double never writes more than 17 significant digits -- so the count is per form of
    # the digit-string generator, and the two repr generators are asserted to stay at 17 or fewer
    for g in ("digits_plain", "digits_point", "digits_exponent"):
        long_ = [t for t in gen[g] if E.significant_digits(t) > 19]
        fl = flags_of(exe, long_)
        assert fl.count(0) >= 20, (g, len(long_), fl.count(0))
    for g in ("repr_bits", "repr_uniform"):
        assert len(gen[g]) >= 5000 and max(E.significant_digits(t) for t in gen[g]) <= 17
        assert sum(flags_of(exe, gen[g])) == 0
    for name, text, ffm, _ in E.hard_numbers():
        r = E.expect(text, ffm)
        lines = text.split("\n")[:-1]
        assert len(r["y"]) == len(lines) == len(r["data"]), name
        if name.startswith("hard_numbers"):
            # every token once as a target and once as a value (the flagged ones twice: both ends of the list)
            assert [ln.split(" ")[0] for ln in lines] == toks and [ln.rsplit(":", 1)[1] for ln in lines] == toks[::-1]
            assert len(text) > 5 * E.TILE
            first, last = text[:E.TILE], text[-E.TILE:]
            for t in flagged:  # in the first tile and in one beyond the fourth, as a target and as a value
                assert "\n" + t + " " in "\n" + first and ":" + t + "\n" in first, t
                assert "\n" + t + " " in last and ":" + t + "\n" in last, t
    many = [c for c in E.hard_numbers() if c[0] == "many_flagged_svm"][0][1]
    mids = E.flagged_midpoints(E.N_MANY_FLAGGED)
    assert len(set(mids)) == E.N_MANY_FLAGGED and sum(flags_of(exe, mids)) == E.N_MANY_FLAGGED >= 5000
    assert len(many) // E.TILE > 16  # pushed from many workgroups of both kernels
    lines = many.split("\n")[:-1]
    assert [ln.split(" ")[0] for ln in lines] == mids and [ln.rsplit(":", 1)[1] for ln in lines] == mids[::-1]


def test_beyond_one_pass():
    name, text, ffm, _, r = E.beyond_one_pass()
    assert isinstance(text, bytes) and E.BEYOND_LINES == 4194304 + 300
    period = E.PERIOD
    assert period.count("\n") == E.PERIOD_LINES == 4 and period.count(":") == E.PERIOD_ENTRIES == 5
    plines = period.split("\n")[:-1]
    assert "" in plines and any(ln and ":" not in ln for ln in plines) and plines[0][0].isdigit()  # empty, target-only, first has a target
    reps = len(text) // len(period)
    assert text == period.encode() * reps and reps * 4 == E.BEYOND_LINES
    assert len(r["y"]) == E.BEYOND_LINES > E.GRID_CAP            # k_lines goes round (it runs n_lines + 1 threads' worth)
    assert len(r["data"]) == reps * 5 > 5_200_000 > E.GRID_CAP    # k_entries and k_narrow go round
    n_tiles = (len(text) + E.TILE - 1) // E.TILE
    assert n_tiles > E.TILE_GRID_CAP + 256 and len(text) < 160e6  # k_tile_counts and k_tile_positions go round too
    assert all(E.significant_digits(t) <= 19 for t in period.replace(":", " ").split())  # none for the fix-up list
    # the tiling is the oracle's result: three periods through the oracle itself
    three = E.expect(period * 3, ffm)
    tiled = E.tiled_expectation(E.expect(period, ffm), 3)
    for key in ("indptr", "indices", "data", "y"):
        assert np.array_equal(three[key], tiled[key]), key
    assert three["n_features"] == tiled["n_features"] == r["n_features"]
    assert np.array_equal(r["indptr"][-4:], r["indptr"][-5] + np.array([3, 3, 3, 5])) and r["indptr"][-1] == len(r["data"])


def test_refusals():
    for name, text, ffm, exc, pattern, span in E.refusals():
        if span is None:
            assert len(text) > 6 * E.TILE, name
            if exc == "ValueError":
                with pytest.raises(ValueError, match="Negative index"):
                    E.expect(text, ffm)
            continue
        a, b = span
        first = text[a:b]
        assert first in (E.BAD_FFM if ffm else E.BAD_SVM) and text[a - 1] == "\n" and text[b] == "\n", name
        assert a // E.TILE == 1, name
        # exactly two lines differ from the well-formed text, in different tiles
        good = list(E.body_lines(ffm, 4800, 2))
        lines = text.split("\n")[:-1]
        diff = [i for i, (g, l) in enumerate(zip(good, lines)) if g != l]
        assert len(diff) == 2 and lines[diff[0]] == first, name
        second = sum(len(ln) + 1 for ln in lines[:diff[1]])
        assert second // E.TILE == 5, name
        if ffm:
            assert text.count(":") % 2 == 0 and first.count(":") == 1 and lines[diff[1]].count(":") == 1, name
    name, text, ffm, exc, pattern, span = E.too_many_flagged()
    line = text[:text.index(b"\n") + 1]
    assert text == line * (len(text) // len(line)) and 2 * (len(text) // len(line)) > E.MAX_FIX
    assert line.decode().split(" ")[0] == E.FLAGGED[0] and line.decode().strip().rsplit(":", 1)[1] == E.FLAGGED[0]
    assert 55e6 < len(text) < 65e6 and str(2 * (len(text) // len(line))) in pattern


def test_the_oracle_accepts_every_well_formed_case():
    for name, text, ffm, kw in E.well_formed_cases():
        r = E.expect(text, ffm, **kw)
        assert len(r["y"]) > 0 and r["indptr"][-1] == len(r["data"]) == len(r["indices"]), name
        assert r["n_features"] >= 1 and (not ffm or (r["n_fields"] >= 1 and len(r["fields"]) == len(r["data"]))), name
