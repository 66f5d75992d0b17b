"""The restatement of the reference's dataset procs (tests/dataset_ops_restatement.py) held to an independent dense numpy
computation: on the reference's own 4 x 6 literal (tests/golden/ref_dataset_literal.json, test_dataset.nim:124-128) with the
checks of test_dataset.nim:228-276, and on the random cases the GPU test uses (tests/dataset_ops_cases.py).  Also pins what
those cases must contain."""
import json
import os

import numpy as np
import pytest

import dataset_ops_cases as K
import dataset_ops_restatement as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def to_csr(dense, y=None):
    """toCSRMatrix: the non-zeros of every row in column order"""
    indptr, indices, data = [0], [], []
    for row in dense:
        for j, v in enumerate(row):
            if v != 0.0:
                indices.append(j)
                data.append(v)
        indptr.append(len(indices))
    return R.Csr(indptr, indices, data, len(dense), len(dense[0]), y=y)


def dense_of(X):
    """dense matrix with repeated ids ADDED (so that it is defined for every case), fields as a second matrix"""
    A = np.zeros((X.n, X.d))
    for i in range(X.n):
        for q in range(X.indptr[i], X.indptr[i + 1]):
            A[i, X.indices[q]] += X.data[q]
    return A


def dense_norm(A, axis, norm):
    """normalizeL1 / L2 / Linfty of the reference's tests on a dense matrix (numpy's own sums: compared with a tolerance)"""
    B = np.abs(A)
    nv = {"l1": B.sum(axis=axis), "l2": np.sqrt((A * A).sum(axis=axis)), "linfty": B.max(axis=axis, initial=0.0)}[norm]
    nv = np.where(nv == 0.0, 1.0, nv)
    return A / (nv[:, None] if axis == 1 else nv[None, :])


@pytest.fixture(scope="module")
def literal():
    with open(os.path.join(GOLD, "ref_dataset_literal.json")) as f:
        g = json.load(f)
    return g["data"], g["yTrue"]


def test_literal_slices_and_selections(literal):
    data, y = literal
    X, A = to_csr(data, y), np.array(data)
    n = len(data)
    for i in range(n - 1):
        for j in range(i + 1, n):
            S = R.slice_rows(X, i, j)
            assert np.array_equal(np.array(S.dense()), A[i:j]) and S.y == y[i:j]
    for rows in ([1, 0, 2], [3, 1]):
        S = R.select_rows(X, rows)
        assert np.array_equal(np.array(S.dense()), A[rows]) and S.y == [y[r] for r in rows]
    # 1..^1 and 0..^2 (dataset.nim:333-335: a ..< nSamples - b + 1)
    assert np.array_equal(np.array(R.slice_rows(X, 1, n).dense()), A[1:])
    assert np.array_equal(np.array(R.slice_rows(X, 0, n - 1).dense()), A[: n - 1])


def test_literal_vstack_and_norms(literal):
    data, y = literal
    X, A = to_csr(data, y), np.array(data)
    V = R.vstack([X, X, X])
    assert np.array_equal(np.array(V.dense()), np.vstack([A, A, A])) and V.y == y * 3 and V.indptr[-1] == 3 * X.nnz
    H = R.hstack([X, X])
    assert np.array_equal(np.array(H.dense()), np.hstack([A, A])) and H.y == y
    for norm in ("l1", "l2", "linfty"):
        for axis in (0, 1):
            N = R.normalize(X, axis, norm)
            np.testing.assert_allclose(np.array(N.dense()), dense_norm(A, axis, norm), rtol=4e-16, atol=0)
            assert N.indices == X.indices and N.indptr == X.indptr and X.data == to_csr(data).data  # a copy


def test_error_texts(literal):
    X = to_csr(literal[0])
    for rows, text in (([], "Invalid slice: nSamples < 1."), ([0, 4], "max(indicesRow) 4 >= 4."), ([2, -1], "min(indicesRow) -1 < 0.")):
        with pytest.raises(ValueError) as e:
            R.select_rows(X, rows)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="Invalid slice"):
        R.slice_rows(X, 2, 2)
    Y = R.Csr([0, 1], [0], [1.0], 1, 5)
    with pytest.raises(ValueError) as e:
        R.vstack([X, Y])
    assert str(e.value) == "All matrics must have the same shape[1]."
    with pytest.raises(ValueError) as e:
        R.hstack([X, Y])
    assert str(e.value) == "All matrics must have the same shape[0]."


def test_forward_draw_is_a_permutation_in_the_reference_order():
    draws = []

    def rand(mx):
        draws.append(mx)
        return (7 * len(draws)) % (mx + 1)

    p = R.forward_draw(9, rand)
    assert draws == list(range(8, -1, -1)) and sorted(p) == list(range(9))
    # by hand: every j = 0 leaves the identity, every j = max reverses pairs from the front
    assert R.forward_draw(5, lambda mx: 0) == [0, 1, 2, 3, 4]
    assert R.forward_draw(4, lambda mx: mx) == [3, 0, 1, 2]


def test_random_cases_against_dense():
    X, S = K.main_case(), K.side_case()
    A, B = dense_of(X), dense_of(S)
    for name, rows in K.selections().items():
        T = R.select_rows(X, rows)
        assert np.array_equal(dense_of(T), A[rows]), name
        assert T.y == [X.y[r] for r in rows] and T.d == X.d
    for a, b in K.SLICES:
        assert np.array_equal(dense_of(R.slice_rows(X, a, b)), A[a:b])
    assert np.array_equal(dense_of(R.hstack([X, S])), np.hstack([A, B]))
    assert np.array_equal(dense_of(R.hstack([S, X, S])), np.hstack([B, A, B]))
    assert np.array_equal(dense_of(R.vstack([X, R.slice_rows(X, 3, 9), X])), np.vstack([A, A[3:9], A]))
    # the norms need distinct ids per row for the dense computation to mean the same thing
    rows = K.selections()["trainable"]
    T = R.select_rows(X, rows)
    for norm in ("l1", "l2", "linfty"):
        for axis in (0, 1):
            np.testing.assert_allclose(dense_of(R.normalize(T, axis, norm)), dense_norm(A[rows], axis, norm), rtol=1e-14, atol=0)


def test_field_cases_against_dense():
    F3, F5, F4 = K.field_cases()
    assert (F3.n_fields, F5.n_fields, F4.n_fields) == (3, 5, 4)
    V = R.vstack([F3, F5, F4])
    assert V.n_fields == 5 and V.fields == F3.fields + F5.fields + F4.fields and V.y is None and V.n == 105
    assert R.vstack([F3, F5]).y == F3.y + F5.y
    H = R.hstack([F3, F5])
    assert H.n_fields == 8 and H.d == 60 and H.y == F3.y
    assert np.array_equal(dense_of(H), np.hstack([dense_of(F3), dense_of(F5)]))
    # fields as a dense matrix of field + 1: part two's are offset by part one's n_fields
    def field_dense(X, off=0):
        A = np.zeros((X.n, X.d))
        for i in range(X.n):
            for q in range(X.indptr[i], X.indptr[i + 1]):
                A[i, X.indices[q]] = X.fields[q] + 1 + off
        return A
    FH = field_dense(H)
    assert np.array_equal(FH[:, :30], field_dense(F3))
    assert np.array_equal(FH[:, 30:], np.where(field_dense(F5) > 0, field_dense(F5, 3), 0.0))
    S = R.select_rows(F5, [7, 7, 0])
    assert S.n_fields == 5 and np.array_equal(field_dense(S), field_dense(F5)[[7, 7, 0]])


def test_cases_contain_what_they_are_meant_to():
    X, S = K.main_case(), K.side_case()
    lens = [X.indptr[i + 1] - X.indptr[i] for i in range(X.n)]
    assert X.n == 300 and X.d >= 256
    for row, want in K.SPECIAL_LEN.items():
        assert lens[row] == want
    sel = K.selections()
    assert len(set(sel["repeats_a_row"])) < len(sel["repeats_a_row"]) and K.ROW_200 in sel["repeats_a_row"]
    assert sel["reversed"] == sorted(sel["reversed"], reverse=True) and len(sel["reversed"]) == X.n
    assert R.select_rows(X, sel["zero_entries"]).nnz == 0
    assert R.select_rows(X, sel["long_rows"]).nnz >= 64 * len(sel["long_rows"])  # the copy kernels' wavefront-per-row path
    assert all(R.select_rows(X, sel[name]).nnz < 64 * len(sel[name]) for name in ("reversed", "random_80_percent", "trainable"))  # 8 lanes per row
    assert K.ROW_REPEAT in sel["repeats_a_row"] and K.ROW_REPEAT not in sel["trainable"] and K.ROW_200 in sel["trainable"]
    # a repeated id in exactly one row; some row stored out of column order
    rep = [i for i in range(X.n) if len(set(X.indices[X.indptr[i]:X.indptr[i + 1]])) < lens[i]]
    assert rep == [K.ROW_REPEAT]
    assert any(X.indices[q] > X.indices[q + 1] for i in range(X.n) for q in range(X.indptr[i], X.indptr[i + 1] - 1))
    # zero norms: the row and the column hold stored zeros only, and are left as they are (0 / 0 would be NaN)
    for norm in ("l1", "l2", "linfty"):
        N1, N0 = R.normalize(X, 1, norm), R.normalize(X, 0, norm)
        assert N1.data[X.indptr[K.ROW_ZERO_NORM]:X.indptr[K.ROW_ZERO_NORM + 1]] == [0.0, 0.0, 0.0]
        col = [q for q in range(X.nnz) if X.indices[q] == K.COL_ZERO_NORM]
        assert len(col) == 2 and all(N0.data[q] == 0.0 for q in col)
        assert not any(np.isnan(N1.data)) and not any(np.isnan(N0.data))
    rows_of_col = {i for i in range(X.n) for q in range(X.indptr[i], X.indptr[i + 1]) if X.indices[q] == K.COL_MANY_ROWS}
    assert len(rows_of_col) >= 65
    # hstack: one part's row empty, the other's not, both ways
    slen = [S.indptr[i + 1] - S.indptr[i] for i in range(S.n)]
    assert lens[K.ROW_63] > 0 and slen[K.ROW_63] == 0 and lens[K.ROW_EMPTY] == 0 and slen[K.ROW_EMPTY] > 0
    F3, F5, _ = K.field_cases()
    assert F3.n_fields != F5.n_fields and F3.fields is not None


@pytest.mark.parametrize("name,text,bad", K.RATING_TEXTS, ids=[t[0] for t in K.RATING_TEXTS])
def test_rating_texts(name, text, bad):
    if bad:
        with pytest.raises(ValueError):
            R.load_user_item(text)
        return
    X = R.load_user_item(text)
    # independent reading: the first three digit runs of every line of five characters or more
    import re
    rows = [re.findall(r"\d+(?:\.\d+)?(?:[eE][+-]?\d+)?", ln) for ln in text.replace("\r", "").split("\n") if len(ln) >= 5]
    ints = [re.findall(r"\d+", ln) for ln in text.replace("\r", "").split("\n") if len(ln) >= 5]
    users, items = [int(r[0]) for r in ints], [int(r[1]) for r in ints]
    assert X.n == len(users) and X.indptr == [2 * i for i in range(X.n + 1)] and X.data == [1.0] * (2 * X.n)
    mu, mi = min(1, min(users)), min(1, min(items))
    nu = max(users) - mu + 1
    assert X.d == nu + max(items) - mi + 1
    assert X.indices[0::2] == [u - mu for u in users] and X.indices[1::2] == [nu + i - mi for i in items]
    if name not in ("multi_space", "comma_float"):  # the third number is a plain one there
        assert X.y == [float(r[2]) for r in rows]
    expect_base = {"one_based": (1, 1), "zero_based": (0, 0), "smallest_id_5": (1, 1)}.get(name)
    if expect_base:
        assert (mu, mi) == expect_base
    if name == "smallest_id_5":
        assert X.d == 9 + 7 and X.indices[:2] == [4, 9 + 6]
    if name == "multi_space":
        assert X.y == [3.25, 4.0]
    if name == "comma_float":
        assert X.y == [4.5, 0.5]
