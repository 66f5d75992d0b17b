"""The restatements of tests/stream_file_restatement.py against each other and against the reference's documented quirks:
what tests/test_gpu_stream_files.py compares the device code with.  No GPU."""
import math
import struct

import numpy as np
import pytest

import stream_file_restatement as R


def grid():
    """a few hundred matrices of at most 12 x 9: unsorted rows, empty interior and trailing records, repeated ids"""
    rng = np.random.default_rng(2024)
    for case in range(300):
        n, d = int(rng.integers(1, 13)), int(rng.integers(1, 10))
        k = int(rng.integers(0, 3))
        empty = set(int(r) for r in rng.choice(n, min(k, n - 1), replace=False)) if n > 1 else set()
        if case % 3 == 0 and n > 1:
            empty.add(n - 1)  # a trailing empty record
        if len(empty) >= n:
            empty = set()
        yield R.random_records(rng, n, d, float(rng.uniform(0.1, 0.8)), empty=empty, repeats=case % 5 == 0) + (n, d)


def test_literal_at_a_whole_matrix_cache_is_the_plain_transposition():
    count = 0
    for indptr, indices, data, n, d in grid():
        x = R.write_stream(indptr, indices, data, None, "csr", n, d, vmax=123.0, vmin=-7.0)
        t = R.transpose_literal(x, len(data))
        assert t == R.transpose_plain(x)
        assert t[:9] == b"STREAMCSC" and t[9:49] == x[9:49]  # the header as it is: max / min, nRows / nCols unswapped
        count += 1
    assert count == 300


def test_a_smaller_cache_is_no_behaviour_to_copy():
    """the literal restatement at caches of 1, 2 and nnz / 3 entries: wrong bytes, an index error or no end on 427 of the 900
    cases (DESIGN.md section 30 quotes the figure), which is why the hosts accept cacheSize and ignore it"""
    bad = total = 0
    for indptr, indices, data, n, d in grid():
        x = R.write_stream(indptr, indices, data, None, "csr", n, d)
        want = R.transpose_plain(x)
        for cache in (1, 2, max(1, len(data) // 3)):
            total += 1
            try:
                ok = R.transpose_literal(x, cache, max_passes=2000) == want
            except (IndexError, R.DoesNotTerminate):
                ok = False
            bad += not ok
    assert (bad, total) == (427, 900)


def test_csr_to_csc_to_csr_sorts_the_rows_by_column_stably():
    for indptr, indices, data, n, d in grid():
        x = R.write_stream(indptr, indices, data, None, "csr", n, d)
        c = R.transpose_literal(x, len(data))
        rows_nonempty_first = indptr[1] > indptr[0]
        if not rows_nonempty_first:
            with pytest.raises(R.DoesNotTerminate):
                R.transpose_literal(c, len(data), max_passes=50)
            continue
        back = R.transpose_literal(c, len(data))
        kind, _, ip2, idx2, val2 = R.read_plain(back)
        assert kind == "csr" and np.array_equal(ip2, indptr)
        for r in range(n):
            a, b = indptr[r], indptr[r + 1]
            order = np.argsort(indices[a:b], kind="stable")
            assert np.array_equal(idx2[a:b], indices[a:b][order])
            assert np.array_equal(val2[a:b], data[a:b][order])


def test_an_empty_first_output_record_does_not_terminate():
    rng = np.random.default_rng(5)
    indptr, indices, data = R.random_records(rng, 6, 5, 0.5, first_id_present=False)
    keep = indices != 0  # no entry with id 0: output record 0 is empty
    counts = [int(keep[indptr[r]:indptr[r + 1]].sum()) for r in range(6)]
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices, data = indices[keep], data[keep]
    assert len(data) > 0
    x = R.write_stream(indptr, indices, data, None, "csr", 6, 5)
    with pytest.raises(R.DoesNotTerminate):
        R.transpose_literal(x, len(data), max_passes=50)
    empty = R.write_stream(np.zeros(4, dtype=np.int64), [], [], None, "csr", 3, 2)  # nnz = 0
    with pytest.raises(R.DoesNotTerminate):
        R.transpose_literal(empty, 0, max_passes=50)


FFM = {
    0: "1 0:0:0.5 2:3:-1.25\n-1 1:1:2\n0 2:0:1e-3 0:2:7\n",
    1: "1 1:1:0.5 3:4:-1.25\n-1 2:2:2\n0 3:1:1e-3 1:3:7\n",
    3: "1 1:3:0.5 3:6:-1.25\n-1 2:4:2\n0 3:3:1e-3 1:5:7\n",  # fields 1-based, smallest index 3
}


@pytest.mark.parametrize("base", [0, 1, 3])
def test_convert_ffm_shifts_the_ids_and_not_the_fields(base):
    xb, yb = R.convert_ffm(FFM[base])
    assert xb[:14] == b"STREAMCSRFIELD"
    n, d, nnz, nf, mx, mn = struct.unpack_from("<qqqqdd", xb, 14)
    # minIndex starts at 1 (:1209): a file whose smallest index is 3 is shifted by 1, not by 3, and nCols counts from 1
    assert (n, d, nnz, mx, mn) == (3, 6 if base == 3 else 4, 5, 7.0, -1.25)
    recs, pos = [], 62
    for _ in range(n):
        (c,) = struct.unpack_from("<q", xb, pos)
        pos += 8
        recs.append([struct.unpack_from("<qdq", xb, pos + 24 * e) for e in range(c)])
        pos += 24 * c
    assert pos == len(xb)
    ids = [[e[2] for e in r] for r in recs]
    fields = [[e[0] for e in r] for r in recs]
    assert ids == ([[2, 5], [3], [2, 4]] if base == 3 else [[0, 3], [1], [0, 2]])  # shifted by minIndex = min(1, smallest)
    if base == 0:
        # minFieldIndex = 0, maxFieldIndex = 2: nFields = 3, and the fields stay below it
        assert nf == 3 and fields == [[0, 2], [1], [2, 0]]
    else:
        # minFieldIndex stays 1 (its initial value), maxFieldIndex = 3: nFields = 3, and a field EQUAL to nFields is written
        assert nf == 3 and fields == [[1, 3], [2], [3, 1]]
    assert np.array_equal(np.frombuffer(yb, dtype="<f8"), [1.0, -1.0, 0.0])


def test_convert_ffm_errors_in_the_reference_order():
    with pytest.raises(ValueError, match="Negative field index is included."):
        R.convert_ffm("1 -1:-2:0.5\n")  # both negative: the field is reported
    with pytest.raises(ValueError, match="Negative index is included."):
        R.convert_ffm("1 0:-2:0.5\n")


def bits(v):
    return struct.pack("<d", v)


def test_header_fold_is_ordered():
    mx, mn = R.fold_min_max([0.0, -0.0, 1.0])
    assert bits(mn) == bits(0.0) and mx == 1.0
    mx, mn = R.fold_min_max([-0.0, 0.0])
    assert bits(mn) == bits(-0.0) and bits(mx) == bits(-0.0)
    mx, mn = R.fold_min_max([float("nan"), 2.0, float("nan"), -3.0])
    assert (mx, mn) == (2.0, -3.0)
    mx, mn = R.fold_min_max([float("nan")])
    assert mx == -math.inf and mn == math.inf
    assert R.fold_min_max([]) == (-math.inf, math.inf)
    x = R.write_stream([0, 2], [0, 1], [-0.0, 0.0], None, "csc", 2, 1)
    assert x[:9] == b"STREAMCSC" and x[33:41] == bits(-0.0) and x[41:49] == bits(-0.0)
