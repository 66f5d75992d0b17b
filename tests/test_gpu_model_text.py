"""The number blocks of a model dump parsed on the device (nfm_parse_f64 / parseF64, nimfm_amd/csrc/model_text.hip, DESIGN.md
section 31) against Python's float() on every token (tests/model_text_cases.py).  Values are compared as bytes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi

import model_text_cases as MC

pytestmark = pytest.mark.gpu

# the kernels' constants, mirrored; test_constants_are_the_kernels holds them to the source
K_TILE = 16384
GRID_CAP = 1024
MAX_FIX = 1 << 20


def parse(text, n_rows, row_len, chunk=0):
    """-> (rc, clean, consumed, values as bytes)"""
    out = np.full(max(n_rows * row_len, 1), -777.0)
    consumed, clean = C.c_int64(-1), C.c_int32(-1)
    rc = capi.lib().nfm_parse_f64(nf.default_context().h, text, len(text), n_rows, row_len, chunk, out.ctypes.data_as(C.c_void_p),
                                  C.byref(consumed), C.byref(clean))
    return rc, clean.value, consumed.value, out[: n_rows * row_len].tobytes()


def assert_parses(text, n_rows, row_len, chunk=0, want=None):
    ok, consumed, vals = want or MC.expect(text, n_rows, row_len)
    assert ok
    rc, clean, got_consumed, got = parse(text, n_rows, row_len, chunk)
    assert (rc, clean) == (capi.NFM_OK, 1)
    assert got_consumed == consumed
    if got != vals:
        a, b = np.frombuffer(got, dtype=np.uint64), np.frombuffer(vals, dtype=np.uint64)
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError("value %d of %d: %016x, float() gives %016x" % (i, len(a), a[i], b[i]))


def test_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc", "model_text.hip")).read()
    assert re.search(r"constexpr int kMtChunk = 64;", src) and re.search(r"constexpr int kMtTile = kBlock \* kMtChunk;", src)
    assert K_TILE == 256 * 64
    assert re.search(r"constexpr int kMtGridCap = %d;" % GRID_CAP, src)
    assert re.search(r"constexpr int kMtMaxFix = 1 << 20;", src)


@pytest.mark.parametrize("name", sorted(MC.clean_cases()))
def test_clean(name):
    text, n_rows, row_len = MC.clean_cases()[name]
    assert_parses(text, n_rows, row_len)
    got = nf.parseF64(text, n_rows, row_len)
    ok, consumed, vals = MC.expect(text, n_rows, row_len)
    assert got[1] == consumed and got[0].shape == (n_rows, row_len) and got[0].tobytes() == vals


def test_parse_f64_takes_buffers():
    text, n_rows, row_len = MC.clean_cases()["text_goes_on"]
    _, consumed, vals = MC.expect(text, n_rows, row_len)
    for buf in (bytearray(text), memoryview(text), memoryview(b"xx" + text)[2:], np.frombuffer(text, dtype=np.uint8)):
        got = nf.parseF64(buf, n_rows, row_len)
        assert got[1] == consumed and got[0].tobytes() == vals
    out = np.zeros((n_rows, row_len))
    assert nf.parseF64(text, n_rows, row_len, out=out)[0] is out and out.tobytes() == vals


@pytest.mark.parametrize("name", sorted(MC.not_clean_cases()))
def test_not_clean(name):
    text, n_rows, row_len = MC.not_clean_cases()[name]
    assert not MC.expect(text, n_rows, row_len)[0]
    for chunk in (0, 2048):
        rc, clean, _, _ = parse(text, n_rows, row_len, chunk)
        assert (rc, clean) == (capi.NFM_OK, 0)
    assert nf.parseF64(text, n_rows, row_len) is None


def test_not_clean_in_a_later_piece():
    rows = [["%d" % (7 * r + c) for c in range(8)] for r in range(400)]
    for damage in (lambda r: r[:-1], lambda r: r[:3] + ["4x"] + r[4:]):
        for at in (0, 200, 399):
            bad = [damage(r) if i == at else r for i, r in enumerate(rows)]
            text = MC.lines_of(bad)
            for chunk in (0, 256):
                rc, clean, _, _ = parse(text, 400, 8, chunk)
                assert (rc, clean) == (capi.NFM_OK, 0), (at, chunk)
    assert_parses(MC.lines_of(rows), 400, 8, 256)


@functools.lru_cache(maxsize=None)
def base_block():
    """512 lines of 8 numbers and what float() makes of them"""
    text = MC.block_of(MC.random_doubles(4096, seed=5), 512, 8)
    return text, np.frombuffer(MC.expect(text, 512, 8)[2], dtype=np.float64).reshape(512, 8)


def text_of_length(n_bytes):
    """lines of 8 numbers, n_bytes long to the byte: whole copies of the base block, some more of its lines, spaces before the
    last newline.  -> (text, rows, values as bytes) with float()'s values"""
    base, vals = base_block()
    reps = n_bytes // len(base)
    ends = [i + 1 for i, c in enumerate(base) if c == 10]
    rest = n_bytes - reps * len(base)
    more = max([0] + [j + 1 for j, e in enumerate(ends) if e <= rest])
    text = base * reps + base[: ends[more - 1] if more else 0]
    assert text, "shorter than one line"
    text = text[:-1] + b" " * (n_bytes - len(text)) + b"\n"
    assert len(text) == n_bytes
    return text, reps * 512 + more, b"".join([vals.tobytes()] * reps + [vals[:more].tobytes()])


@pytest.mark.parametrize("n_bytes", [K_TILE - 1, K_TILE, K_TILE + 1, 3 * K_TILE + 5, (GRID_CAP + 1) * K_TILE],
                         ids=["tile-1", "tile", "tile+1", "3tiles+5", "grid_cap+1_tiles"])
def test_tile_and_grid_edges(n_bytes):
    text, rows, vals = text_of_length(n_bytes)
    assert_parses(text, rows, 8, 0, want=(True, n_bytes, vals))
    if n_bytes > 4 * K_TILE:  # more tokens than one trip of the token kernel's grid: 1024 workgroups of 256
        assert rows * 8 > GRID_CAP * 256
    # the same text as one row: every token of a long line finds its column
    flat = text.replace(b"\n", b" ")[:-1] + b"\n"
    assert_parses(flat, 1, rows * 8, 0, want=(True, n_bytes, vals))


def test_separators_on_tile_edges():
    def pad(line, end):  # the line's '\n' at byte end - 1
        return line + b" " * (end - 1 - len(line)) + b"\n"
    a = pad(b"1.5 2.5 0.5", K_TILE)                       # '\n' on the last byte of tile 0
    b = b"3.5 4.5" + b" " * (K_TILE - 7 - 1) + b"7"   # a token on the first byte of tile 1, one on its last byte
    c = b"\n" + b"8.5 9.5 6\n"                        # '\n' on the first byte of tile 2
    text = a + b + c
    assert text[K_TILE - 1] == 10 and text[K_TILE] == ord("3") and text[2 * K_TILE - 1] == ord("7") and text[2 * K_TILE] == 10
    assert text[2 * K_TILE - 2] == 32
    assert_parses(text, 3, 3)
    for chunk in (K_TILE, K_TILE + 1, 2 * K_TILE, 2 * K_TILE + 1):
        assert_parses(text, 3, 3, chunk)
    # a token that straddles the tile edge, and one that starts on the text's first and ends on its last byte
    text = b"1" + b" " * (K_TILE - 4) + b"123.456789 5\n6 7"
    assert text[K_TILE - 1] == ord("3") and text[K_TILE] == ord(".")
    assert_parses(text, 2, 2)


def test_chunks_of_the_small_block():
    text = MC.BLOCK_3x40
    want = MC.expect(text, 3, 40)
    for chunk in range(32, 97):
        assert_parses(text, 3, 40, chunk, want=want)


@functools.lru_cache(maxsize=None)
def mb_block():
    text = MC.block_of(MC.random_doubles(300 * 330, seed=6), 300, 330)
    return text, MC.expect(text, 300, 330)


@pytest.mark.parametrize("chunk", [97, 4096, 0])
def test_chunks_of_a_block_of_megabytes(chunk):
    text, want = mb_block()
    assert len(text) > 2 << 20
    assert_parses(text + b"w:\n1 2 3\n", 300, 330, chunk, want=want)


def test_stats_and_timing_families():
    text, want = mb_block()
    ctx = nf.default_context()
    ctx.timing_enable(True)
    ctx.timing_reset()
    assert_parses(text, 300, 330, 1 << 18, want=want)
    pieces, nbytes = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().nfm_parse_stats(C.byref(pieces), C.byref(nbytes), None, None, None))
    launches = ctx.timing_get("load_index")[0], ctx.timing_get("load_parse")[0]
    ctx.timing_enable(False)
    assert nbytes.value == len(text) and pieces.value >= -(-len(text) // (1 << 18)) > 8
    assert launches[0] >= pieces.value and launches[1] >= pieces.value


def test_invalid_arguments():
    L, h = capi.lib(), nf.default_context().h
    out = np.zeros(4)
    vp = out.ctypes.data_as(C.c_void_p)
    consumed, clean = C.c_int64(0), C.c_int32(0)
    cp, kp = C.byref(consumed), C.byref(clean)
    t = b"1 2\n3 4\n"
    assert L.nfm_parse_f64(h, t, len(t), 2, 2, 0, vp, cp, kp) == capi.NFM_OK and clean.value == 1
    for args in ((None, t, len(t), 2, 2, 0, vp, cp, kp), (h, None, len(t), 2, 2, 0, vp, cp, kp), (h, t, len(t), 2, 2, 0, None, cp, kp),
                 (h, t, len(t), 2, 2, 0, vp, None, kp), (h, t, len(t), 2, 2, 0, vp, cp, None), (h, t, -1, 2, 2, 0, vp, cp, kp),
                 (h, t, len(t), -2, 2, 0, vp, cp, kp), (h, t, len(t), 2, -2, 0, vp, cp, kp), (h, t, len(t), 2, 2, -1, vp, cp, kp),
                 (h, t, len(t), 1 << 62, 4, 0, vp, cp, kp), (h, t, len(t), 1 << 40, 1 << 40, 0, vp, cp, kp)):
        assert L.nfm_parse_f64(*args) == capi.ERR_INVALID, args[2:6]
    # nothing to parse needs no text and no values
    assert L.nfm_parse_f64(h, None, 0, 0, 5, 0, None, cp, kp) == capi.NFM_OK and (consumed.value, clean.value) == (0, 1)
    assert L.nfm_parse_f64(h, None, 0, 1, 1, 0, vp, cp, kp) == capi.NFM_OK and clean.value == 0


def test_fix_list_cap():
    tok = b"1.000000000000000111022302462515654042363166809082031251"  # float() rounds up; 19 digits cannot tell
    want = np.float64(float(tok))
    assert want == 1.0000000000000002
    n = MAX_FIX
    text = (tok + b" ") * n + b"\n"
    rc, clean, consumed, vals = parse(text, 1, n)
    assert (rc, clean, consumed) == (capi.NFM_OK, 1, len(text))
    assert np.array_equal(np.frombuffer(vals, dtype=np.float64), np.full(n, want))
    text = (tok + b" ") * (n + 1) + b"\n"
    rc, clean, _, _ = parse(text, 1, n + 1)
    assert (rc, clean) == (capi.NFM_OK, 0)  # more than the list holds: left to the caller
