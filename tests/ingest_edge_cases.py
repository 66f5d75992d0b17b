"""The inputs shared by tests/test_ingest_edge_cases.py (CPU) and tests/test_gpu_ingest_edges.py: svmlight / libffm texts
built so that their delimiters, their ends and their line and entry counts fall on the structural edges of ingest.hip -- the
8-byte words, 16-byte loads and 64-byte chunks of the '\\n' / ':' scan inside its 16-KiB tiles, the end-of-text mask of
load_chunk64, rows and runs of empty lines longer than a tile, the launch cap of grid_for (16384 x 256 threads), the number
parser's hard tokens and the strtod fix-up list.

Pure Python and numpy.  A case is a tuple (name, text, with_fields, kwargs); what the GPU must deliver for it is
oracle.ingest.load_svmlight / load_ffm of the same text (expect() below).  The periodic texts that are too long for the
oracle's Python loop come with the oracle's result for one period tiled by numpy (tiled_expectation()).  A refusal is a
tuple (name, text, with_fields, exception name, message pattern, span): span is the byte range [a, b) of the first malformed
line where the message names a byte.

What each family is meant to reach is asserted on the built texts by tests/test_ingest_edge_cases.py."""
import decimal
import functools
import random
import struct

import numpy as np

from oracle import ingest

TILE = 16384            # kTile = kBlock * kChunk (ingest.hip)
CHUNK = 64              # kChunk: bytes per thread
GRID_CAP = 16384 * 256  # grid_for: at most 256 * 64 workgroups of kBlock threads
MAX_FIX = 1 << 20       # kMaxFix

# token tables whose periods (7, 11, 5, 9, 3) are coprime to 64 and to each other
TARGETS = ["1", "-1", "0.5", "-2.25", "1e-3", "12.125", "-0.0625"]
COUNTS = [3, 0, 5, 1, 8, 2, 4, 6, 1, 7, 3]  # entries per line
IDS = ["3", "41", "507", "6", "29"]         # unsorted and repeated inside a line: ingest accepts both
VALS = ["1", "0.5", "-2", "3.25", "1e-3", "-0.125", "7.0625", "2.5e+10", "-6"]
FLDS = ["1", "2", "13"]


def expect(text, with_fields, **kwargs):
    return ingest.load_ffm(text, **kwargs) if with_fields else ingest.load_svmlight(text, **kwargs)


@functools.lru_cache(maxsize=None)
def body_lines(ffm, n, phase=0):
    """n well-formed lines (no terminators) whose lengths and token lengths cycle through the tables above"""
    out, c = [], phase
    for i in range(n):
        s = TARGETS[(i + phase) % len(TARGETS)]
        for _ in range(COUNTS[(i + phase) % len(COUNTS)]):
            s += " " + (FLDS[c % len(FLDS)] + ":" if ffm else "") + IDS[c % len(IDS)] + ":" + VALS[c % len(VALS)]
            c += 1
        out.append(s)
    return tuple(out)


def pad_target(n):
    """a decimal of exactly n >= 1 characters (a target-only line of n + 1 bytes)"""
    if n < 3:
        return "17"[:n] if n == 2 else "7"
    return ("0." + "1234567895" * (n // 10 + 1))[:n]


def positions(text, ch):
    b = np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8)
    return np.nonzero(b == ord(ch))[0]


# ---------------------------------------------------------------- delims_at_every_offset
def _first_colon_of_its_entry(body, p):
    return body.rfind(" ", 0, p) > body.rfind(":", 0, p)


def place(body, ch, at, first_of_entry=False):
    """body behind one target-only line whose length puts an occurrence of ch at byte `at`"""
    p = at - 2
    while p >= 0 and not (body[p] == ch and (not first_of_entry or _first_colon_of_its_entry(body, p))):
        p -= 1
    assert p >= 0
    text = pad_target(at - p - 1) + "\n" + body
    assert text[at] == ch
    return text


def delims_at_every_offset():
    cases = []
    for ffm in (False, True):
        body = "\n".join(body_lines(ffm, 2400, 1 if ffm else 0)) + "\n"
        fmt = "ffm" if ffm else "svm"
        for ch, what in (("\n", "newline"), (":", "colon")):
            for at in (TILE - 1, TILE):
                cases.append(("delims_%s_%s_at_%d" % (fmt, what, at), place(body, ch, at), ffm, {}))
        if ffm:  # the two colons of one entry on opposite sides of the tile edge
            cases.append(("delims_ffm_entry_across_%d" % TILE, place(body, ":", TILE - 1, first_of_entry=True), True, {}))
    return cases


# ---------------------------------------------------------------- length_sweep / dirty_padding
SWEEP_LENGTHS = list(range(1, 81)) + list(range(TILE - 72, TILE + 73))
ENDINGS = ("newline", "no_newline", "colon_at_len_minus_2")
_TAIL = {"newline": "\n", "no_newline": "", "colon_at_len_minus_2": " 5:7"}


def exact_length_text(length, ending):
    """a well-formed svmlight text of exactly `length` bytes: whole lines of body_lines, then one target whose digit count
    makes up the length, then the ending.  None where the ending does not fit (`<t> 5:7` needs 5 bytes)."""
    tail = _TAIL[ending]
    parts, used = [], 0
    for ln in body_lines(False, 700):
        if used + len(ln) + 1 + 1 + len(tail) > length:
            break
        parts.append(ln + "\n")
        used += len(ln) + 1
    n = length - used - len(tail)
    if n == 0 and ending == "newline" and not parts:
        return "\n"  # length 1: one empty line
    if n < 1:
        return None
    text = "".join(parts) + pad_target(n) + tail
    assert len(text) == length
    return text


@functools.lru_cache(maxsize=None)
def length_sweep():
    cases = []
    for length in SWEEP_LENGTHS:
        for ending in ENDINGS:
            text = exact_length_text(length, ending)
            if text is not None:
                cases.append(("length_%d_%s" % (length, ending), text, False, {}))
    return tuple(cases)


DIRT_UNIT = ":\n"


def dirt(nbytes=1 << 20):
    """nothing but delimiters: malformed on purpose, parsed to leave them in the block the next text is given"""
    return DIRT_UNIT * (nbytes // 2)


# ---------------------------------------------------------------- long_rows
LONG_ROW_LENGTHS = [1, 3000, 0, 0, 1, 9000, 1]


def long_rows():
    cases = []
    for ffm in (False, True):
        rng = np.random.default_rng(17)
        lines, q = [], 0
        for i, m in enumerate(LONG_ROW_LENGTHS):
            mant = rng.integers(-99, 100, size=m)
            dec = rng.integers(-8, 8, size=m)  # the decade spread of random_csr_text(wide=True)
            full = rng.uniform(-1, 1, size=m) * 10.0 ** dec
            s = repr(float(i) - 2.5)
            for j in range(m):
                idx = (q * 7919) % 97 + 1  # unsorted, repeated
                val = repr(float(full[j])) if j % 10 == 9 else "%de%d" % (mant[j], dec[j])
                s += " " + ("%d:" % (q % 5 + 1) if ffm else "") + "%d:%s" % (idx, val)
                q += 1
            lines.append(s)
        cases.append(("long_rows_%s" % ("ffm" if ffm else "svm"), "\n".join(lines) + "\n", ffm, {}))
    return cases


# ---------------------------------------------------------------- empty_runs
EMPTY_RUNS = (700, 20000, 513)


def empty_runs():
    cases = []
    for sep in ("\n", "\r\n"):
        for first in ("1.5", "1.25"):
            lines = [first] + [""] * EMPTY_RUNS[0] + ["-1 3:0.5 1:2"] + [""] * EMPTY_RUNS[1] + ["2 7:1 7:2"] + [""] * EMPTY_RUNS[2]
            text = sep.join(lines) + sep
            if sep == "\n" or (text[TILE - 1] == "\r" and text[TILE] == "\n"):
                break
        cases.append(("empty_runs_%s" % ("lf" if sep == "\n" else "crlf"), text, False, {}))
    return cases


# ---------------------------------------------------------------- hard_numbers
# tests/test_parse_num.py's HARD list, the forms the parser accepts whole
HARD = ["0", "-0.0", "1", "1.5", "0.1", "0.30000000000000004", "1e22", "1e23", "9007199254740993", "9007199254740992.5",
        "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "1.7976931348623157e308",
        "1.7976931348623159e308", "1e309", "1e-400", "123456789012345678901234567890", "0.000001", "5e-324",
        "2.2250738585072014e-308", "2.2250738585072011e-308",
        "1.00000000000000011102230246251565404236316680908203125",
        "1.00000000000000011102230246251565404236316680908203124",
        "1.00000000000000011102230246251565404236316680908203126", ".5", "5.", "+3.25", "1E5", "1e+5", "1e-5",
        "8.41e21", "nan", "inf", "-inf", "Infinity"]
# tokens for which the host build of parse_num.h returns flag 1 (checked by the CPU test): the device lists them for strtod
FLAGGED = ["1.00000000000000011102230246251565404236316680908203125", "2.4703282292062327208051355972e-324",
           "0.500000000000000166533453693773481063544750213623046875"]
GENERATORS = ("digits_plain", "digits_point", "digits_exponent", "repr_bits", "repr_uniform")


def significant_digits(tok):
    """as tests/test_parse_num.py counts them"""
    return len("".join(c for c in tok.lower().split("e")[0] if c.isdigit()).lstrip("0"))


@functools.lru_cache(maxsize=None)
def generated_tokens(n_digits=9000, n_bits=6000, n_uniform=5000, seed=1):
    """the three random generators of tests/test_parse_num.py -> {generator: [tokens]}; the digit strings are kept apart
    by their form (plain, with a point, with a point and an exponent)"""
    rnd = random.Random(seed)
    out = {g: [] for g in GENERATORS}
    for _ in range(n_digits):
        nd = rnd.randint(1, 22)
        digs = "".join(rnd.choice("0123456789") for _ in range(nd))
        kind = rnd.random()
        p = rnd.randint(0, nd)
        t = digs if kind < 0.3 else digs[:p] + "." + digs[p:]
        if kind >= 0.7:
            t += "e" + str(rnd.randint(-330, 310))
        t = ("-" if rnd.random() < 0.3 else "") + t
        out["digits_plain" if kind < 0.3 else "digits_point" if kind < 0.7 else "digits_exponent"].append(t)
    while len(out["repr_bits"]) < n_bits:
        x = struct.unpack("<d", struct.pack("<Q", rnd.getrandbits(64)))[0]
        if x == x and abs(x) != float("inf"):
            out["repr_bits"].append(repr(x))
    for _ in range(n_uniform):
        out["repr_uniform"].append(repr(rnd.uniform(-1, 1)))
    return out


def _number_text(tokens, ffm):
    """line i: token i as the target, token n - 1 - i as the value of its one entry"""
    n = len(tokens)
    pre = ["%d:" % (i % 3 + 1) if ffm else "" for i in range(3)]
    return "\n".join("%s %s%d:%s" % (tokens[i], pre[i % 3], (i * 13) % 41 + 1, tokens[n - 1 - i]) for i in range(n)) + "\n"


def hard_number_tokens():
    flagged = FLAGGED + ["-" + t for t in FLAGGED]
    gen = generated_tokens()
    return flagged + HARD + [t for g in GENERATORS for t in gen[g]] + flagged


def flagged_midpoints(n, seed=7):
    """n decimals that sit on, just above or just below the midpoint of two neighbouring doubles in [0.5, 2), written out
    exactly (53 or more digits): the 19-digit truncation w and w + 1 round to different doubles, so each takes the fix-up"""
    rnd = random.Random(seed)
    out = []
    with decimal.localcontext() as ctx:
        ctx.prec = 120
        while len(out) < n:
            x = rnd.uniform(0.5, 2.0)
            up = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] + 1))[0]
            mid = (decimal.Decimal(x) + decimal.Decimal(up)) / 2
            s = format(mid, "f")
            k = len(out) % 3
            if k:  # the last digit of an exact midpoint is 5: one up or one down
                s = s[:-1] + ("6" if k == 1 else "4")
            out.append(("-" if len(out) % 5 == 4 else "") + s)
    return out


N_MANY_FLAGGED = 5000


def hard_numbers():
    cases = []
    for ffm in (False, True):
        cases.append(("hard_numbers_%s" % ("ffm" if ffm else "svm"), _number_text(hard_number_tokens(), ffm), ffm, {}))
    # value and target alternate in the text: line i holds tokens i (target) and n - 1 - i (value)
    cases.append(("many_flagged_svm", _number_text(flagged_midpoints(N_MANY_FLAGGED), False), False, {}))
    return cases


# ---------------------------------------------------------------- beyond_one_pass
# four lines, five entries; the first line has a target, so the empty second line repeats a value of its own period.  The
# numbers are written with 17 digits (none takes the fix-up) so that the text is longer than the tile kernels' one trip
PERIOD = ("1.5000000000000002 3:0.12345678901234568 7:-1.2345678901234567e-03 2:4.0000000000000009\n\n-2.5\n"
          "0.125 1:1.0000000000000002 9:0.50000000000000011\n")
PERIOD_LINES, PERIOD_ENTRIES = 4, 5
BEYOND_LINES = GRID_CAP + 300
TILE_GRID_CAP = 256 * 32  # text_line_index: at most that many workgroups walk the tiles


def tiled_expectation(r, reps):
    """the oracle's result r for one period -> its result for `reps` periods in a row"""
    nnz = int(r["indptr"][-1])
    indptr = np.concatenate([[0], (r["indptr"][1:][None, :] + nnz * np.arange(reps, dtype=np.int64)[:, None]).ravel()])
    out = dict(r)
    out.update(indptr=indptr, indices=np.tile(r["indices"], reps), data=np.tile(r["data"], reps), y=np.tile(r["y"], reps))
    if "fields" in r:
        out["fields"] = np.tile(r["fields"], reps)
    return out


def beyond_one_pass():
    """-> (name, text as bytes, with_fields, kwargs, expectation).  More lines than one launch of k_lines has threads and
    more tiles than k_tile_counts / k_tile_positions have workgroups (8192 tiles = 128 MiB), so k_lines, k_entries, k_narrow
    and both tile kernels go round their loops."""
    assert BEYOND_LINES % PERIOD_LINES == 0
    reps = BEYOND_LINES // PERIOD_LINES
    return ("beyond_one_pass", PERIOD.encode() * reps, False, {}, tiled_expectation(expect(PERIOD, False), reps))


# ---------------------------------------------------------------- refusals
BAD_SVM = ["1 1:0.5junk", "1 a:0.5", "1  1:2", "2:3 1:1"]  # the last: "2:3" glued to the line start, no target
BAD_FFM = ["1 1:0.5", "-1 2:7"]  # one colon each: the total stays even, only the per-line check and the pairing see it


def two_bad_lines(ffm, first, second, tile_a=1, tile_b=5):
    """a well-formed text of more than six tiles with one line in tile_a and one in tile_b replaced -> (text, span of the first)"""
    lines = list(body_lines(ffm, 4800, 2))
    start = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])])
    ia = int(np.searchsorted(start, tile_a * TILE + 700))
    ib = int(np.searchsorted(start, tile_b * TILE + 700))
    lines[ib] = second  # replaced first: the offsets before it do not move
    lines[ia] = first
    text = "\n".join(lines) + "\n"
    a = int(start[ia])
    assert text[a:a + len(first) + 1] == first + "\n"
    return text, (a, a + len(first))


def refusals():
    out = []
    for i, bad in enumerate(BAD_SVM):
        text, span = two_bad_lines(False, bad, BAD_SVM[(i + 1) % len(BAD_SVM)])
        out.append(("two_bad_svm_%d" % i, text, False, "ValueError", r"malformed svmlight text: (\d+) bad tokens, first near byte (\d+)", span))
    for i, bad in enumerate(BAD_FFM):
        text, span = two_bad_lines(True, bad, BAD_FFM[1 - i])
        out.append(("two_bad_ffm_%d" % i, text, True, "ValueError", r"malformed libffm text: (\d+) bad tokens, first near byte (\d+)", span))
    late = list(body_lines(False, 4800, 2))
    late[4000] = "1 3000000000:1"
    out.append(("id_3000000000", "\n".join(late) + "\n", False, "NfmError", r"feature index 3000000000 does not fit int32", None))
    late[4000] = "1 4:1 -3:2"
    out.append(("negative_id_late_tile", "\n".join(late) + "\n", False, "ValueError", r"Negative index is included", None))
    return out


def too_many_flagged():
    """more tokens for the fix-up list than kMaxFix: refused by count before any of them is copied (about 60 MB)"""
    line = ("%s 1:%s\n" % (FLAGGED[0], FLAGGED[0])).encode()
    n_lines = MAX_FIX // 2 + 1
    return ("too_many_flagged", line * n_lines, False, "NfmError", r"%d tokens with more than 19 significant digits" % (2 * n_lines), None)


def well_formed_cases():
    """every well-formed case but the sweep (length_sweep()) and the one built by multiplication (beyond_one_pass())"""
    return delims_at_every_offset() + long_rows() + empty_runs() + hard_numbers()
