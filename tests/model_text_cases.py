"""Texts for the parser of a model dump's number blocks (nfm_parse_f64, nimfm_amd/csrc/model_text.hip and its serial walk in
model_text_pieces.h), shared by tests/test_cpp_model_text_pieces.py (CPU) and tests/test_gpu_model_text.py.

The expected value of a token is Python's float() on it -- a correctly rounded strtod -- compared as bytes, so that the sign
of a zero and of a NaN counts.  What is CLEAN is restated here from the rule, not taken from the code under test: the block
is the first n_rows lines; a token is a maximal run of bytes other than ' ' and '\\n'; every token of the block, those beyond
row_len too, has to be a number in parse_float's syntax to its last byte, and every line needs row_len tokens at least."""
import re

import numpy as np

from nimfm_amd.host import _nim_float

# [+-] digits [. digits] [(e|E) [+-] digits] | [+-] nan | [+-] inf[inity]   (nimfm_amd/csrc/parse_num.h)
NUMBER = re.compile(rb"[+-]?(?:[nN][aA][nN]|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)")
MAX_TOKEN = 1024

REPR_TOKENS = [repr(v) for v in (0.0, -0.0, 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e+308,
                                 1e22, 1e23, 0.30000000000000004, 1e-05, 1e+20)]
HAND_TOKENS = ["+1.5", "1.", ".5", "1E5", "1e+05", "-0", "00012.50", "1e-400", "1e400",
               "9007199254740993",
               "1.00000000000000011102230246251565404236316680908203125",
               "1.000000000000000111022302462515654042363166809082031251",
               "1234567890123456789012",
               "0.1000000000000000055511151231257827021181583404541015625",
               "nan", "-nan", "+nan", "NAN", "inf", "-inf", "+inf", "Infinity", "-infinity"]
TOKENS = REPR_TOKENS + HAND_TOKENS


def random_doubles(n, seed=20):
    """n finite doubles drawn as uniform 64-bit patterns"""
    rng = np.random.default_rng(seed)
    out = np.zeros(0)
    while len(out) < n:
        v = rng.integers(0, 2 ** 64, 2 * n, dtype=np.uint64).view(np.float64)
        out = np.concatenate([out, v[np.isfinite(v)]])
    return out[:n]


def lines_of(rows):
    """rows of token strings -> the text a dump writes: one space between, "\\n" after every row"""
    return "".join(" ".join(r) + "\n" for r in rows).encode("ascii")


def block_of(values, n_rows, row_len):
    toks = [_nim_float(v) for v in values]
    return lines_of([toks[r * row_len:(r + 1) * row_len] for r in range(n_rows)])


def expect(text, n_rows, row_len):
    """-> (clean, consumed, values as bytes): the rule, with float() as the reader"""
    pos, rows = 0, []
    for _ in range(n_rows):
        if pos >= len(text):
            return False, None, None  # fewer than n_rows lines
        e = text.find(b"\n", pos)
        line, pos = (text[pos:], len(text)) if e < 0 else (text[pos:e], e + 1)
        rows.append([t for t in line.split(b" ") if t])
    vals = np.zeros((n_rows, row_len))
    for r, toks in enumerate(rows):
        if len(toks) < row_len or any(len(t) > MAX_TOKEN or not NUMBER.fullmatch(t) for t in toks):
            return False, None, None
        vals[r] = [float(t) for t in toks[:row_len]]
    return True, pos, vals.tobytes()


BLOCK_3x40 = block_of(random_doubles(120, seed=3), 3, 40)


def clean_cases():
    """name -> (text, n_rows, row_len)"""
    t = TOKENS
    rnd = random_doubles(4096)
    c = {
        "tokens_one_row": (lines_of([t]), 1, len(t)),
        "tokens_one_per_row": (lines_of([[v] for v in t]), len(t), 1),
        "tokens_rows_of_4": (lines_of([t[i:i + 4] for i in range(0, len(t), 4)]), len(t) // 4, 4),
        "random_64x64": (block_of(rnd, 64, 64), 64, 64),
        "random_1x4096": (block_of(rnd, 1, 4096), 1, 4096),
        "random_4096x1": (block_of(rnd, 4096, 1), 4096, 1),
        "block_3x40": (BLOCK_3x40, 3, 40),
        "1x1": (b"1.5\n", 1, 1),
        "1x2": (b"1.5 -2\n", 1, 2),
        "2x1": (b"1.5\n-2\n", 2, 1),
        "3x5": (lines_of([["%d.25" % (5 * r + s) for s in range(5)] for r in range(3)]), 3, 5),
        "double_spaces": (b"1  2   3\n4  5  6\n", 2, 3),
        "leading_space": (b" 1 2\n  3 4\n", 2, 2),
        "space_before_newline": (b"1 2 \n3 4  \n", 2, 2),
        "extra_tokens": (b"1 2 3 4\n5 6 7\n", 2, 2),
        "extra_tokens_row_len_1": (b"1 2 3 4\n5 6 7\n", 2, 1),
        "text_goes_on": (b"1 2\n3 4\nw:\n0.5 0.25\nintercept: 1\n", 2, 2),
        "text_goes_on_with_junk": (b"1 2\nabc \t\r 1_0\n", 1, 2),
        "no_final_newline": (b"1 2\n3 4", 2, 2),
        "no_final_newline_one_row": (b"7", 1, 1),
        "no_final_newline_space": (b"1 2\n3 4 ", 2, 2),
        "zero_rows": (b"1 2\n", 0, 2),
    }
    return c


def not_clean_cases():
    return {
        "short_first_row": (b"1\n3 4\n5 6\n", 3, 2),
        "short_middle_row": (b"1 2\n3\n5 6\n", 3, 2),
        "short_last_row": (b"1 2\n3 4\n5\n", 3, 2),
        "short_last_row_open": (b"1 2\n3 4\n5", 3, 2),
        "too_few_lines": (b"1 2\n3 4\n", 3, 2),
        "too_few_lines_by_two": (b"1 2\n", 3, 2),
        "empty_text": (b"", 1, 1),
        "abc": (b"1 abc\n", 1, 2),
        "1.0x": (b"1.0x 2\n", 1, 2),
        "5e": (b"5e 2\n", 1, 2),
        "1_0": (b"1_0 2\n", 1, 2),
        "crlf": (b"1.0 2.0\r\n3.0 4.0\r\n", 2, 2),
        "tab": (b"1\t2\n", 1, 2),
        "tab_beside_space": (b"1 \t2\n", 1, 2),
        "empty_line": (b"1 2\n\n3 4\n", 3, 2),
        "junk_beyond_row_len": (b"1 2 x\n", 1, 2),
        "lone_sign": (b"1 -\n", 1, 2),
        "lone_point": (b". 1\n", 1, 2),
        "nul_byte": (b"1 \x00 2\n", 1, 2),
        "token_too_long": (b"1 " + b"0" * (MAX_TOKEN + 1) + b"\n", 1, 2),
    }
