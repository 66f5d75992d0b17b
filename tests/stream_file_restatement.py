"""TEST INFRASTRUCTURE ONLY -- plain-Python restatements of the reference's writers of its binary stream format
(tensor/sparse_stream.nim:3-33), shared by tests/test_stream_file_restatement.py (no GPU) and tests/test_gpu_stream_files.py:

    transpose_literal   transposeFile, dataset.nim:1100-1199, line by line, at a cache of n_cached_max elements
    transpose_plain     what it computes when the cache holds every entry, said directly
    convert_ffm         convertFFMFile, dataset.nim:1202-1299, on oracle.ingest's parse_int / parse_float
    write_stream        a file of either kind from its arrays, with the header's ordered min / max fold

Nothing here is imported by the product path.
"""
import struct

import numpy as np

from oracle.ingest import _lines, parse_float, parse_int

MAGIC = {"csr": b"STREAMCSR", "csc": b"STREAMCSC", "csrfield": b"STREAMCSRFIELD"}


def fold_min_max(values):
    """-> (max, min) as dataset.nim:1021-1022, 1052-1053 fold them from -Inf / +Inf, spelled as the library's own host code
    did before the device packer (v < vmin ? v : vmin): a NaN never replaces a bound, and of values that compare equal
    (+0.0 / -0.0) the first in storage order stays."""
    vmin, vmax = float("inf"), float("-inf")
    for v in values:
        v = float(v)
        vmin = v if v < vmin else vmin
        vmax = v if v > vmax else vmax
    return vmax, vmin


def write_stream(indptr, indices, data, fields, kind, n_rows, n_cols, n_fields=0, vmax=None, vmin=None):
    """the bytes of a STREAMCSR / STREAMCSC / STREAMCSRFIELD file whose records are indptr's segments.  n_rows / n_cols go
    into the header as given (a STREAMCSC file carries nSamples / nFeatures, unswapped); max / min are the ordered fold
    over data unless given."""
    fmax, fmin = fold_min_max(data)
    vmax = fmax if vmax is None else vmax
    vmin = fmin if vmin is None else vmin
    x = bytearray(MAGIC[kind])
    if kind == "csrfield":
        x += struct.pack("<qqqqdd", n_rows, n_cols, len(data), n_fields, vmax, vmin)
    else:
        x += struct.pack("<qqqdd", n_rows, n_cols, len(data), vmax, vmin)
    for r in range(len(indptr) - 1):
        x += struct.pack("<q", int(indptr[r + 1] - indptr[r]))
        for q in range(int(indptr[r]), int(indptr[r + 1])):
            if kind == "csrfield":
                x += struct.pack("<qdq", int(fields[q]), float(data[q]), int(indices[q]))
            else:
                x += struct.pack("<dq", float(data[q]), int(indices[q]))
    return bytes(x)


def read_plain(xbytes):
    """-> (kind, header bytes, indptr, indices, data) of a plain file; the records are rows (csr) or columns (csc)"""
    kind = "csr" if xbytes[:9] == MAGIC["csr"] else "csc" if xbytes[:9] == MAGIC["csc"] else None
    if kind is None:
        raise IOError("is not neither StreamCSC nor StreamCSR file.")
    n_rows, n_cols, _ = struct.unpack_from("<qqq", xbytes, 9)
    n_rec = n_rows if kind == "csr" else n_cols
    pos, indptr, indices, data = 49, [0], [], []
    for _ in range(n_rec):
        (c,) = struct.unpack_from("<q", xbytes, pos)
        pos += 8
        for _ in range(c):
            v, i = struct.unpack_from("<dq", xbytes, pos)
            pos += 16
            data.append(v)
            indices.append(i)
        indptr.append(len(indices))
    return kind, xbytes[9:49], np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(data, dtype=np.float64)


class DoesNotTerminate(RuntimeError):
    pass


def transpose_literal(xbytes, n_cached_max, max_passes=1000):
    """transposeFile (dataset.nim:1100-1199) statement by statement, with nCachedElementsMax given directly instead of being
    derived from cacheSize (:1134-1135).  The `while j < header.nCols` loop is capped at max_passes passes: DoesNotTerminate
    where the reference would loop for ever.  Nim's index errors are Python's IndexError."""
    magic = xbytes[:9]
    if magic == MAGIC["csr"]:
        out = bytearray(MAGIC["csc"])
    elif magic == MAGIC["csc"]:
        out = bytearray(MAGIC["csr"])
    else:
        raise IOError("is not neither StreamCSC nor StreamCSR file.")
    header = xbytes[9:49]
    out += header  # :1122-1124
    n_rows, n_cols, _ = struct.unpack_from("<qqq", header)
    if magic == MAGIC["csc"]:
        n_rows, n_cols = n_cols, n_rows  # :1127-1128
    nnz_cols = [0] * n_cols
    nnz_cols_rest = [0] * n_cols
    offsets = [0] * n_cols
    elements = [None] * n_cached_max
    body = 49
    pos = body
    for _ in range(n_rows):  # :1138-1142
        (nnz,) = struct.unpack_from("<q", xbytes, pos)
        pos += 8
        for _ in range(nnz):
            _, eid = struct.unpack_from("<dq", xbytes, pos)
            pos += 16
            if eid < 0:
                raise IndexError(eid)
            nnz_cols[eid] += 1
    for j in range(n_cols):
        nnz_cols_rest[j] = nnz_cols[j]
    j = 0
    last_read = -1
    out += struct.pack("<q", nnz_cols[0])  # :1150
    passes = 0
    while j < n_cols:
        passes += 1
        if passes > max_passes:
            raise DoesNotTerminate("transposeFile: %d passes and j = %d of %d" % (max_passes, j, n_cols))
        n_cached_cols = 0
        pos = body
        n_cached_rest = n_cached_max
        while j + n_cached_cols < n_cols:  # :1157-1165
            offsets[j + n_cached_cols] = n_cached_max - n_cached_rest
            n_cached_rest -= nnz_cols_rest[j + n_cached_cols]
            if n_cached_rest >= 0:
                nnz_cols_rest[j + n_cached_cols] = 0
                n_cached_cols += 1
            else:
                nnz_cols_rest[j + n_cached_cols] = -n_cached_rest
                break
        n_cached = 0
        last_read_next = 0
        for i in range(n_rows):  # :1170-1188
            if n_cached == n_cached_max:
                break
            (nnz_row,) = struct.unpack_from("<q", xbytes, pos)
            pos += 8
            for _ in range(nnz_row):
                val, eid = struct.unpack_from("<dq", xbytes, pos)
                pos += 16
                if eid >= j and eid <= j + n_cached_cols:
                    if eid == j and i <= last_read:
                        continue
                    if eid == j + n_cached_cols:
                        if offsets[eid] >= n_cached_max:
                            continue
                        else:
                            last_read_next = i
                    elements[offsets[eid]] = (val, i)
                    offsets[eid] += 1
                    n_cached += 1
        for ii in range(n_cached):  # :1190-1196
            out += struct.pack("<dq", elements[ii][0], elements[ii][1])
            nnz_cols[j] -= 1
            while j < n_cols and nnz_cols[j] == 0:
                j += 1
                if j < n_cols:
                    out += struct.pack("<q", nnz_cols[j])
        last_read = last_read_next
    return bytes(out)


def transpose_plain(xbytes):
    """the other magic, the header as it is, and output record j = the entries with id j by ascending input record, entries
    of one input record that repeat j in storage order"""
    kind, header, indptr, indices, data = read_plain(xbytes)
    n_rows, n_cols, _ = struct.unpack_from("<qqq", header)
    n_out = n_cols if kind == "csr" else n_rows
    cols = [[] for _ in range(n_out)]
    for r in range(len(indptr) - 1):
        for q in range(indptr[r], indptr[r + 1]):
            cols[indices[q]].append((data[q], r))
    out = bytearray(MAGIC["csc" if kind == "csr" else "csr"]) + header
    for c in cols:
        out += struct.pack("<q", len(c))
        for v, r in c:
            out += struct.pack("<dq", v, r)
    return bytes(out)


def convert_ffm(text):
    """convertFFMFile (dataset.nim:1202-1299) -> (bytes of the STREAMCSRFIELD file, bytes of the label file).  ids are shifted
    by minIndex (initial 1), nCols = maxIndex - minIndex + 1; the FIELDS ARE NOT SHIFTED (:1287 against :1294) while
    nFields = maxFieldIndex - minFieldIndex + 1 (initial 1 / 0)."""
    lines = _lines(text)
    min_val, max_val = float("inf"), float("-inf")
    min_index, max_index = 1, 0
    min_field, max_field = 1, 0
    j, field, val, target = 0, 0, 0.0, 0.0
    n_samples = nnz = 0
    for line in lines:
        pos = 0
        n_samples += 1
        c, target = parse_float(line, pos, target)
        pos += c + 1
        while pos < len(line):
            c, field = parse_int(line, pos, field)
            pos += c
            min_field, max_field = min(field, min_field), max(field, max_field)
            pos += 1
            c, j = parse_int(line, pos, j)
            pos += c
            min_index, max_index = min(j, min_index), max(j, max_index)
            pos += 1
            c, val = parse_float(line, pos, val)
            pos += c
            min_val = val if val < min_val else min_val
            max_val = val if val > max_val else max_val
            pos += 1
            nnz += 1
    if min_field < 0:
        raise ValueError("Negative field index is included.")
    if min_index < 0:
        raise ValueError("Negative index is included.")
    x = bytearray(MAGIC["csrfield"])
    x += struct.pack("<qqqqdd", n_samples, max_index - min_index + 1, nnz, max_field - min_field + 1, max_val, min_val)
    y = bytearray()
    for line in lines:
        pos = 0
        c, target = parse_float(line, pos, target)
        pos += c + 1
        y += struct.pack("<d", target)
        row = []
        while pos < len(line):
            c, field = parse_int(line, pos, field)
            pos += c + 1
            c, j = parse_int(line, pos, j)
            pos += c + 1
            c, val = parse_float(line, pos, val)
            pos += c + 1
            row.append((field, val, j - min_index))
        x += struct.pack("<q", len(row))
        for f, v, i in row:
            x += struct.pack("<qdq", f, v, i)
    return bytes(x), bytes(y)


# ---- the matrices both test files use ---------------------------------------------------------------------------------------
def random_records(rng, n, d, density=0.3, empty=(), first_id_present=True, repeats=False):
    """n records over ids < d in UNSORTED storage order; the records listed in `empty` have no entries; first_id_present: id 0
    occurs, so the transposed file's first record is not empty.  -> (indptr, indices, data)"""
    indptr, indices, data = [0], [], []
    for r in range(n):
        if r not in empty:
            m = int(rng.binomial(d, density))
            ids = rng.choice(d, m, replace=False) if not repeats else rng.integers(0, d, m)
            indices += [int(i) for i in ids]
            data += [float(v) for v in np.round(rng.standard_normal(m), 3)]
        indptr.append(len(indices))
    if first_id_present and 0 not in indices:
        r = next(r for r in range(n) if r not in empty)
        at = indptr[r + 1]
        indices.insert(at, 0)
        data.insert(at, 0.5)
        for q in range(r + 1, n + 1):
            indptr[q] += 1
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(data, dtype=np.float64)


def matrix_37x11(rng):
    """37 x 11: an empty first record, empty interior and trailing records, unsorted rows"""
    return random_records(rng, 37, 11, 0.35, empty=(0, 5, 6, 20, 35, 36))


def long_record(rng, d=6000, long_len=5000):
    """records of 0 - 3 entries around one of long_len entries"""
    indptr, indices, data = [0], [], []
    lens = [2, 0, 3, 1, long_len, 0, 1, 3, 2, 0]
    for m in lens:
        ids = rng.choice(d, m, replace=False)
        indices += [int(i) for i in ids]
        data += [float(v) for v in np.round(rng.standard_normal(m), 3)]
        indptr.append(len(indices))
    if 0 not in indices:
        indices[indptr[4]] = 0
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(data, dtype=np.float64)
