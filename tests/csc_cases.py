"""Inputs of the column-major dataset tests, shared by the CPU test of the restatement (tests/test_csc_restatement.py) and
the GPU test of the device code (tests/test_gpu_csc.py).  Everything is drawn once from fixed seeds."""
import json
import os

import numpy as np

from dataset_ops_cases import _rows_to_csr
from dataset_ops_restatement import Csr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dataset_literal.json")

# columns of long_case() with 9, 70 and 1100 entries: more than a lane group's 8, more than a wavefront's 64, more than a
# workgroup's 256 at a time
COL_9, COL_70, COL_1100 = 3, 11, 17


def literal_case():
    """the reference's 4 x 6 matrix and yTrue (tests/test_dataset.nim:124-128): its row 2 and columns 1 are empty"""
    with open(GOLDEN) as f:
        lit = json.load(f)
    dense = lit["data"]
    rows = [[(j, v) for j, v in enumerate(r) if v != 0.0] for r in dense]
    return _rows_to_csr(rows, len(dense), len(dense[0]), y=lit["yTrue"]), dense


def random_rows(seed, n, d, max_len, with_y=True, sort=False):
    """rows of 0 .. max_len entries in no particular column order (sort: ascending)"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        m = int(rng.integers(0, min(max_len, d) + 1))
        cols = rng.choice(d, m, replace=False)
        if sort:
            cols = np.sort(cols)
        rows.append([(int(j), float(rng.uniform(-2, 2))) for j in cols])
    y = [float(v) for v in rng.standard_normal(n)] if with_y else None
    return _rows_to_csr(rows, n, d, y=y)


def small_cases():
    """name -> Csr: the shapes at which a transposition, a filter or a stack can go wrong"""
    lit, _ = literal_case()
    out = {
        "literal": lit,
        "one_row": _rows_to_csr([[(4, 1.5), (0, -2.0), (2, 0.25)]], 1, 5, y=[3.0]),
        "one_column": _rows_to_csr([[(0, 1.0)], [], [(0, -3.5)], [(0, 0.0)]], 4, 1, y=[1.0, 2.0, 3.0, 4.0]),
        "no_entries": _rows_to_csr([[], [], []], 3, 4, y=[0.5, -0.5, 1.5]),
        "empty_rows_and_columns": _rows_to_csr([[], [(5, 1.0), (1, 2.0)], [], [(1, -1.0)], []], 5, 7, y=[1.0, 2.0, 3.0, 4.0, 5.0]),
        "unsorted_rows": random_rows(2501, 37, 23, 9),
        # a row that repeats a column id: the repeats keep the row's storage order inside the column
        "repeat_in_row": _rows_to_csr([[(2, 1.0), (0, 2.0), (2, 3.0), (2, -4.0)], [(2, 5.0)], [(1, 6.0), (1, 7.0)]], 3, 3, y=[1.0, -1.0, 0.5]),
        "wide": random_rows(2502, 9, 41, 12),  # d > n
        "tall": random_rows(2503, 45, 7, 5),  # n > d
        "no_targets": random_rows(2504, 12, 10, 4, with_y=False),
    }
    return out


def repeat_in_column_csc():
    """column arrays (indptr, indices, data, n, d) in which column 1 names sample 2 three times, unsorted: toCSRDataset
    keeps the column-storage order inside row 2"""
    return [0, 2, 7, 7, 8], [3, 0, 2, 0, 2, 1, 2, 3], [1.0, 2.0, 3.0, 4.0, -5.0, 6.0, 7.5, 8.0], 4, 4


def long_case():
    """1300 x 40: columns of 9, 70 and 1100 entries beside one-entry columns and empty ones, rows in no column order"""
    rng = np.random.default_rng(2505)
    n, d = 1300, 40
    want = {COL_9: 9, COL_70: 70, COL_1100: 1100}
    rows = [[] for _ in range(n)]
    for j in range(d):
        m = want.get(j, 1 if j % 3 else 0)
        for i in rng.choice(n, m, replace=False):
            rows[int(i)].append((j, float(rng.uniform(-2, 2))))
    for r in rows:
        rng.shuffle(r)
    rows = [[(int(j), float(v)) for j, v in r] for r in rows]
    return _rows_to_csr(rows, n, d, y=[float(v) for v in rng.standard_normal(n)])


def dense_case():
    """70 x 6 with every entry stored: columns (70) and rows (6) on both sides of the lane-group / wavefront choice once
    transposed (the segments of the column arrays average 70 entries)"""
    rng = np.random.default_rng(2506)
    rows = [[(j, float(rng.uniform(-2, 2))) for j in range(6)] for _ in range(70)]
    return _rows_to_csr(rows, 70, 6, y=[float(v) for v in rng.standard_normal(70)])


def stack_parts(with_targets=True):
    """three parts of 23 columns to vstack (13, 1 and 30 rows) and three parts of 19 rows to hstack (5, 31 and 1 columns)"""
    v = [random_rows(2510 + t, n, 23, 7, with_y=with_targets or t != 1) for t, n in enumerate((13, 1, 30))]
    h = [random_rows(2520 + t, 19, d, 6, with_y=with_targets) for t, d in enumerate((5, 31, 1))]
    return v, h


# (begin, end) of literal_case(): tests/test_dataset.nim:333-340 -- every i ..< j, then 1..^1 and 0..^2
def literal_slices(n=4):
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n)] + [(1, n), (0, n - 1)]


# name -> (text, rows kept as CSC, error expected as CSR)
RATING_TEXTS = {
    "plain": ("1 1 5\n1 3 1\n2 2 3.5\n4 1 2\n", 4, False),
    "four_characters": ("1 1 5\n1 23\n2 3 1\n", 2, True),  # "1 23" is skipped as CSC (:923), refused as CSR
    "short_and_blank": ("a\n1 1 5\nxyz\n\n2 3 1\n3 1 4", 3, False),
}


def trainable_case():
    """80 x 8, distinct ids per row, every row and column used: what the column solvers fit twice"""
    rng = np.random.default_rng(2530)
    n, d = 80, 8
    rows = []
    for i in range(n):
        cols = rng.choice(d, int(rng.integers(1, 5)), replace=False)
        cols = set(int(j) for j in cols) | {i % d}
        rows.append([(j, float(rng.uniform(-1, 1))) for j in rng.permutation(sorted(cols))])
    rows = [[(int(j), v) for j, v in r] for r in rows]
    return _rows_to_csr(rows, n, d, y=[float(v) for v in rng.standard_normal(n)])


def sorted_rows(X):
    """X with every row stably sorted by column id: toCSR(toCSC(X))"""
    indptr, indices, data = [0], [], []
    for i in range(X.n):
        ent = sorted(((X.indices[q], q) for q in range(X.indptr[i], X.indptr[i + 1])))
        indices += [j for j, _ in ent]
        data += [X.data[q] for _, q in ent]
        indptr.append(len(indices))
    return Csr(indptr, indices, data, X.n, X.d, y=X.y)
