"""The restatement of the reference's column-major dataset procs (tests/csc_restatement.py) against dense numpy and against
its own invariants, on the inputs the GPU test (tests/test_gpu_csc.py) holds the device code to."""
import numpy as np
import pytest

import csc_cases as cases
import csc_restatement as R
import dataset_ops_restatement as RR


def _dense(X):
    return np.array(X.dense(), dtype=np.float64).reshape(X.n, X.d)


def _all_cases():
    out = dict(cases.small_cases())
    out["long"] = cases.long_case()
    out["dense"] = cases.dense_case()
    return out


ALL = _all_cases()
NO_REPEATS = [k for k in ALL if k != "repeat_in_row"]


def _check_csc(C):
    assert len(C.indptr) == C.d + 1 and C.indptr[0] == 0 and C.indptr[-1] == C.nnz == len(C.indices)
    assert all(a <= b for a, b in zip(C.indptr, C.indptr[1:]))
    assert all(0 <= i < C.n for i in C.indices)


@pytest.mark.parametrize("name", sorted(ALL))
def test_to_csc_lists_columns_by_ascending_sample(name):
    X = ALL[name]
    C = R.to_csc(X)
    _check_csc(C)
    assert C.y == X.y
    for j in range(C.d):
        ids = C.indices[C.indptr[j]:C.indptr[j + 1]]
        assert ids == sorted(ids)
    if name in NO_REPEATS:
        assert np.array_equal(_dense(C), _dense(X))


@pytest.mark.parametrize("name", sorted(ALL))
def test_round_trip_is_the_stable_sort_of_every_row(name):
    X = ALL[name]
    back = R.to_csr(R.to_csc(X))
    want = cases.sorted_rows(X)
    assert (back.indptr, back.indices, back.data, back.y) == (want.indptr, want.indices, want.data, want.y)


def test_repeats_keep_storage_order_in_both_directions():
    C = R.to_csc(ALL["repeat_in_row"])
    assert C.indptr == [0, 1, 3, 7]
    assert C.indices[3:] == [0, 0, 0, 1] and C.data[3:] == [1.0, 3.0, -4.0, 5.0]
    indptr, indices, data, n, d = cases.repeat_in_column_csc()
    X = R.to_csr(R.Csc(indptr, indices, data, n, d))
    assert X.indptr == [0, 2, 3, 6, 8]
    assert X.indices[3:6] == [1, 1, 1] and X.data[3:6] == [3.0, -5.0, 7.5]
    assert R.column_walk_order(R.Csc(indptr, indices, data, n, d))[2] == [(1, 3.0), (1, -5.0), (1, 7.5)]


@pytest.mark.parametrize("name", sorted(ALL))
def test_column_walk_is_the_row_twin_storage_order(name):
    C = R.to_csc(ALL[name])
    T = R.to_csr(C)
    walk = R.column_walk_order(C)
    for i in range(T.n):
        assert walk[i] == [(T.indices[q], T.data[q]) for q in range(T.indptr[i], T.indptr[i + 1])]


def test_slice_grid_of_the_reference_test():
    """tests/test_dataset.nim:333-340"""
    X, dense = cases.literal_case()
    C = R.to_csc(X)
    for a, b in cases.literal_slices():
        S = R.slice_rows(C, a, b)
        _check_csc(S)
        assert np.array_equal(_dense(S), np.array(dense)[a:b])
        assert S.y == X.y[a:b]


@pytest.mark.parametrize("name", ["unsorted_rows", "long", "tall", "empty_rows_and_columns"])
def test_slice_is_the_columns_of_the_row_slice(name):
    X = ALL[name]
    C = R.to_csc(X)
    for a, b in [(0, X.n), (X.n // 3, X.n // 3 + 1), (X.n // 4, 3 * X.n // 4 + 1)]:
        S = R.slice_rows(C, a, b)
        want = R.to_csc(RR.slice_rows(X, a, b))
        assert (S.indptr, S.indices, S.data, S.y, S.n) == (want.indptr, want.indices, want.data, want.y, want.n)
    for bad in [(2, 2), (0, X.n + 1), (-1, 1)]:
        with pytest.raises(ValueError):
            R.slice_rows(C, *bad)


@pytest.mark.parametrize("with_targets", [True, False])
def test_stacks_against_dense(with_targets):
    v, h = cases.stack_parts(with_targets)
    V = R.vstack([R.to_csc(X) for X in v])
    _check_csc(V)
    assert np.array_equal(_dense(V), np.vstack([_dense(X) for X in v]))
    assert (V.y is not None) == with_targets
    if with_targets:
        assert V.y == [t for X in v for t in X.y]
    # the stack of the columns is the columns of the stack (rows sorted by id first)
    want = R.to_csc(RR.vstack([cases.sorted_rows(X) for X in v]))
    assert (V.indptr, V.indices, V.data) == (want.indptr, want.indices, want.data)
    H = R.hstack([R.to_csc(X) for X in h])
    _check_csc(H)
    assert np.array_equal(_dense(H), np.hstack([_dense(X) for X in h]))
    assert H.y == h[0].y
    with pytest.raises(ValueError, match=r"shape\[1\]\.$"):
        R.vstack([R.to_csc(v[0]), R.to_csc(h[0])])
    with pytest.raises(ValueError, match=r"shape\[0\]$"):
        R.hstack([R.to_csc(h[0]), R.to_csc(v[0])])


def test_vstack_departure_is_a_switch():
    """tensor/sparse.nim:598 sizes indptr by shape[0] + 1: an index error with fewer rows than columns, an unread tail with more"""
    wide = [R.to_csc(ALL["wide"]), R.to_csc(ALL["wide"])]  # 18 rows, 41 columns
    with pytest.raises(IndexError):
        R.vstack(wide, reference_indptr_length=True)
    assert len(R.vstack(wide).indptr) == 42
    tall = [R.to_csc(ALL["tall"]), R.to_csc(ALL["tall"])]  # 90 rows, 7 columns
    ref, dev = R.vstack(tall, reference_indptr_length=True), R.vstack(tall)
    assert len(ref.indptr) == 91 and len(dev.indptr) == 8
    assert ref.indptr[:8] == dev.indptr and set(ref.indptr[8:]) == {dev.indptr[-1]}
    assert (ref.indices, ref.data) == (dev.indices, dev.data)


def _dense_normalized(dense, axis, norm):
    """tests/test_dataset.nim:26-62 normalizeL1 / normalizeL2 / normalizeLinfty, recomputed densely"""
    A = np.array(dense, dtype=np.float64)
    fold = {"l1": lambda v: np.abs(v).sum(), "l2": lambda v: np.sqrt((v * v).sum()), "linfty": lambda v: np.abs(v).max()}[norm]
    out = A.copy()
    for t in range(A.shape[1 - axis]):
        v = A[t, :] if axis == 1 else A[:, t]
        nv = fold(v)
        if nv != 0.0:
            if axis == 1:
                out[t, :] = v / nv
            else:
                out[:, t] = v / nv
    return out


@pytest.mark.parametrize("norm", ["l1", "l2", "linfty"])
@pytest.mark.parametrize("axis", [0, 1])
def test_norms_of_the_reference_test(axis, norm):
    """tests/test_dataset.nim:295-325"""
    X, dense = cases.literal_case()
    N = R.normalize(R.to_csc(X), axis, norm)
    assert np.allclose(_dense(N), _dense_normalized(dense, axis, norm), rtol=1e-15, atol=0)
    # at most two entries per row and column: the fold has one rounding order, so the dense recomputation is exact
    assert np.array_equal(_dense(N), _dense_normalized(dense, axis, norm))


@pytest.mark.parametrize("norm", ["l1", "l2", "linfty"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", ["unsorted_rows", "long", "repeat_in_row"])
def test_normalize_is_the_row_major_fold_on_the_transposed_view(name, axis, norm):
    C = R.to_csc(ALL[name])
    N = R.normalize(C, axis, norm)
    T = RR.normalize(RR.Csr(C.indptr, C.indices, C.data, C.d, C.n), 1 - axis, norm)
    assert N.data == T.data and N.indices == C.indices and N.indptr == C.indptr and N.y == C.y
    if name != "repeat_in_row":
        assert np.allclose(_dense(N), _dense_normalized(ALL[name].dense(), axis, norm), rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", sorted(cases.RATING_TEXTS))
def test_rating_loader_as_csc(name):
    text, kept, csr_refuses = cases.RATING_TEXTS[name]
    C = R.load_user_item_csc(text)
    _check_csc(C)
    assert C.n == kept and C.nnz == 2 * kept and set(C.data) == {1.0}
    if csr_refuses:
        with pytest.raises(ValueError):
            RR.load_user_item(text)
    else:
        want = R.to_csc(RR.load_user_item(text))
        assert (C.indptr, C.indices, C.data, C.y, C.n, C.d) == (want.indptr, want.indices, want.data, want.y, want.n, want.d)
