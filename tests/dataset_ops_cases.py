"""Inputs of the dataset-op tests, shared by the CPU test of the restatement (tests/test_dataset_ops_restatement.py) and the
GPU test of the device code (tests/test_gpu_dataset_ops.py).  Everything is drawn once from fixed seeds."""
import numpy as np

from dataset_ops_restatement import Csr

# special rows of main_case()
ROW_EMPTY, ROW_1, ROW_63, ROW_64, ROW_65, ROW_200, ROW_REPEAT, ROW_ZERO_NORM = 0, 1, 2, 3, 4, 5, 6, 8
COL_MANY_ROWS, COL_ZERO_NORM = 7, 11
SPECIAL_LEN = {ROW_EMPTY: 0, ROW_1: 1, ROW_63: 63, ROW_64: 64, ROW_65: 65, ROW_200: 200}


def _rows_to_csr(rows, n, d, y=None, fields=None, n_fields=0):
    indptr, indices, data, fl = [0], [], [], [] if fields is not None else None
    for i, r in enumerate(rows):
        for t, (j, v) in enumerate(r):
            indices.append(j)
            data.append(v)
            if fl is not None:
                fl.append(fields[i][t])
        indptr.append(len(indices))
    return Csr(indptr, indices, data, n, d, fl, n_fields, y)


def main_case():
    """300 x 260, plain: an empty row; rows of 1, 63, 64, 65 and 200 entries; a row that repeats a column id; a row and a
    column of stored zeros (zero norm); a column present in 90 rows; rows stored in no particular column order."""
    rng = np.random.default_rng(2301)
    n, d = 300, 260
    free = np.array([j for j in range(d) if j not in (COL_MANY_ROWS, COL_ZERO_NORM)])
    rows = []
    for i in range(n):
        m = SPECIAL_LEN.get(i, int(rng.integers(0, 13)))
        cols = rng.choice(free, m, replace=False)  # unsorted
        rows.append([(int(j), float(rng.uniform(-2, 2))) for j in cols])
    rows[ROW_REPEAT] = [(5, 0.75), (9, -1.5), (5, 0.25)]
    rows[ROW_ZERO_NORM] = [(20, 0.0), (COL_ZERO_NORM, 0.0), (21, 0.0)]
    rows[9].append((COL_ZERO_NORM, 0.0))
    for i in range(10, 100):
        rows[i].insert(len(rows[i]) // 2, (COL_MANY_ROWS, float(rng.uniform(-2, 2))))
    return _rows_to_csr(rows, n, d, y=[float(v) for v in rng.standard_normal(n)])


def side_case():
    """300 x 17 to hstack with main_case(): its row ROW_63 is empty where main's is not, its row ROW_EMPTY is not empty"""
    rng = np.random.default_rng(2302)
    n, d = 300, 17
    rows = []
    for i in range(n):
        m = 0 if i == ROW_63 else (3 if i == ROW_EMPTY else int(rng.integers(0, 5)))
        cols = np.sort(rng.choice(d, m, replace=False))
        rows.append([(int(j), float(rng.uniform(-2, 2))) for j in cols])
    return _rows_to_csr(rows, n, d, y=[float(v) for v in rng.standard_normal(n)])


def field_case(seed, n, d, n_fields, with_y=True):
    rng = np.random.default_rng(seed)
    rows, fields = [], []
    for i in range(n):
        m = int(rng.integers(0, 7))
        cols = np.sort(rng.choice(d, m, replace=False))
        rows.append([(int(j), float(rng.uniform(-2, 2))) for j in cols])
        fields.append([int(f) for f in rng.integers(0, n_fields, m)])
    y = [float(v) for v in rng.standard_normal(n)] if with_y else None
    return _rows_to_csr(rows, n, d, y=y, fields=fields, n_fields=n_fields)


def field_cases():
    """field-aware parts with different n_fields: two of 40 x 30 (3 and 5 fields) to stack either way, one of 25 x 30
    without targets for vstack"""
    return field_case(2303, 40, 30, 3), field_case(2304, 40, 30, 5), field_case(2305, 25, 30, 4, with_y=False)


def selections():
    n = 300
    rng = np.random.default_rng(2306)
    no_repeat_row = [i for i in range(n) if i != ROW_REPEAT]
    return {
        "repeats_a_row": [ROW_200, ROW_200, ROW_63, ROW_EMPTY, 299, ROW_REPEAT, ROW_65, ROW_200, ROW_1, ROW_64],
        "reversed": list(range(n - 1, -1, -1)),
        "zero_entries": [ROW_EMPTY, ROW_EMPTY],
        "long_rows": [ROW_200, ROW_65, ROW_64, ROW_200, ROW_63],  # 64 entries per row or more on average: a wavefront per row
        "random_80_percent": [int(i) for i in rng.permutation(n)[: 240]],
        "trainable": [int(i) for i in rng.permutation(no_repeat_row)[: 200]] + [ROW_200],
    }


SLICES = [(0, 300), (0, 1), (1, 7), (ROW_200, ROW_200 + 1), (250, 300)]

# (name, text, error expected)
RATING_TEXTS = [
    ("one_based", "1 1 5\n1 3 1\n2 2 3.5\n4 1 2\n", False),
    ("zero_based", "0 2 4\n3 0 1.5\n1 1 2\n", False),
    ("smallest_id_5", "5 7 3\n9 5 4\n6 6 1\n", False),
    ("double_colon_timestamp", "1::1193::5::978300760\n1::661::3::978302109\n2::1357::5::978298709\n", False),
    ("pipe", "1|3|1\n2|1|4\n", False),
    ("tab", "196\t242\t3\t881250949\n186\t302\t3\t891717742\n", False),
    ("multi_space", "1   2    3.25\n  3  1   4e0  # a comment 7\n", False),
    ("crlf", "1 1 5\r\n2 3 1\r\n", False),
    ("no_final_newline", "1 1 5\n2 3 1", False),
    ("blank_lines", "1 1 5\n\n2 3 1\n\n\n3 2 2\n", False),
    ("short_lines_skipped", "a\n1 1 5\nxyz\n2 3 1\n", False),
    ("comma_float", "10,20,4.5\n11,21,0.5\n", False),
    ("four_characters", "1 1 5\n1 23\n", True),
    ("two_numbers", "1 1 5\n12 34 x\n", True),
    ("nothing", "ab\n\n", True),
]


def svmlight_text(X):
    """X as 1-based svmlight text with its targets (repr round-trips a binary64)"""
    lines = []
    for i in range(X.n):
        ent = " ".join("%d:%r" % (X.indices[q] + 1, X.data[q]) for q in range(X.indptr[i], X.indptr[i + 1]))
        lines.append(("%r %s" % (X.y[i], ent)).rstrip())
    return "\n".join(lines) + "\n"
