"""Plain-Python restatement of the reference's dataset procs, loop for loop in its order, for the device versions
(nimfm_amd/csrc/dataset_ops.hip) to be compared with bit for bit:

    X[indicesRow], X[a..<b]     tensor/sparse.nim:263-285, 333-357; checkIndicesRow dataset.nim:307-316
    shuffle's forward draw      dataset.nim:388-394
    vstack / hstack             tensor/sparse.nim:564-581, 613-633 / :671-698, 719-750
    normalize                   tensor/sparse.nim:372-411
    loadUserItemRatingFile      dataset.nim:840-900

Python floats are binary64 and `+`, `*`, `/`, math.sqrt round once each, as the reference's generated C does without fused
multiply-adds.  Nothing here is vectorised: the order of every sum is the order of the loop.
"""
import math


class Csr:
    """CSRMatrix / CSRFieldMatrix (tensor/sparse.nim:9-24) with the targets the device dataset carries along"""

    def __init__(self, indptr, indices, data, n, d, fields=None, n_fields=0, y=None):
        self.indptr, self.indices, self.data = [int(v) for v in indptr], [int(v) for v in indices], [float(v) for v in data]
        self.n, self.d = int(n), int(d)
        self.fields = None if fields is None else [int(v) for v in fields]
        self.n_fields = int(n_fields) if fields is not None else 0
        self.y = None if y is None else [float(v) for v in y]

    @property
    def nnz(self):
        return len(self.data)

    def dense(self):
        out = [[0.0] * self.d for _ in range(self.n)]
        for i in range(self.n):
            for q in range(self.indptr[i], self.indptr[i + 1]):
                out[i][self.indices[q]] = self.data[q]
        return out


def check_indices_row(X, rows):
    """dataset.nim:307-316"""
    if len(rows) < 1:
        raise ValueError("Invalid slice: nSamples < 1.")
    if max(rows) >= X.n:
        raise ValueError("max(indicesRow) %d >= %d." % (max(rows), X.n))
    if min(rows) < 0:
        raise ValueError("min(indicesRow) %d < 0." % min(rows))


def select_rows(X, rows):
    """tensor/sparse.nim:263-285 (:333-357 with fields); the targets follow the rows"""
    rows = [int(r) for r in rows]
    check_indices_row(X, rows)
    indptr = [0] * (len(rows) + 1)
    nnz = 0
    for ii, i in enumerate(rows):
        nnz += X.indptr[i + 1] - X.indptr[i]
        indptr[ii + 1] = nnz
    indices, data, fields = [0] * nnz, [0.0] * nnz, None if X.fields is None else [0] * nnz
    count = 0
    for i in rows:
        for q in range(X.indptr[i], X.indptr[i + 1]):
            indices[count] = X.indices[q]
            data[count] = X.data[q]
            if fields is not None:
                fields[count] = X.fields[q]
            count += 1
    y = None if X.y is None else [X.y[i] for i in rows]
    return Csr(indptr, indices, data, len(rows), X.d, fields, X.n_fields, y)


def slice_rows(X, a, b):
    """X[a..<b] = X[toSeq(a..<b)] (tensor/sparse.nim:288-290)"""
    return select_rows(X, list(range(a, b)))


def forward_draw(n, rand):
    """dataset.nim:388-394; rand(max) is the generator's rand(max: int), an integer in [0, max]"""
    indices = list(range(n))
    for i in range(n):
        j = rand(n - 1 - i)
        indices[i], indices[i + j] = indices[i + j], indices[i]
    return indices


def vstack(parts):
    """tensor/sparse.nim:564-581, 613-633"""
    first = parts[0]
    indptr, indices, data = list(first.indptr), list(first.indices), list(first.data)
    fields = None if first.fields is None else list(first.fields)
    n, n_fields = first.n, first.n_fields
    for X in parts[1:]:
        nnz = len(data)
        if X.d != first.d:
            raise ValueError("All matrics must have the same shape[1].")
        data += X.data
        indices += X.indices
        indptr += [nnz + v for v in X.indptr[1:]]
        if fields is not None:
            fields += X.fields
            n_fields = max(n_fields, X.n_fields)
        n += X.n
    y = None
    if all(X.y is not None for X in parts):
        y = [v for X in parts for v in X.y]
    return Csr(indptr, indices, data, n, first.d, fields, n_fields, y)


def hstack(parts):
    """tensor/sparse.nim:671-698, 719-750"""
    first = parts[0]
    n, d, n_fields = first.n, first.d, first.n_fields
    for X in parts[1:]:
        if X.n != n:
            raise ValueError("All matrics must have the same shape[0].")
        d += X.d
        n_fields += X.n_fields
    with_fields = first.fields is not None
    indptr, indices, data, fields = [0] * (n + 1), [], [], [] if with_fields else None
    for i in range(n):
        offset = offset_fields = 0
        for X in parts:
            for q in range(X.indptr[i], X.indptr[i + 1]):
                data.append(X.data[q])
                indices.append(X.indices[q] + offset)
                if with_fields:
                    fields.append(X.fields[q] + offset_fields)
                indptr[i + 1] += 1
            offset += X.d
            offset_fields += X.n_fields
    for i in range(n):  # cumsum
        indptr[i + 1] += indptr[i]
    return Csr(indptr, indices, data, n, d, fields, n_fields, first.y)


def _nim_max(x, y):
    return x if y <= x else y  # system.nim: `if y <= x: x else: y`


NORMS = {
    "l1": (lambda x, y: x + abs(y), lambda x: x),
    "l2": (lambda x, y: x + y * y, math.sqrt),
    "linfty": (lambda x, y: _nim_max(x, abs(y)), lambda x: x),
}


def normalize(X, axis, norm):
    """tensor/sparse.nim:372-411 into a copy"""
    f, g = NORMS[norm]
    data = list(X.data)
    if axis == 1:
        for i in range(X.n):
            nv = 0.0
            for q in range(X.indptr[i], X.indptr[i + 1]):
                nv = f(nv, data[q])
            nv = g(nv)
            if nv != 0.0:
                for q in range(X.indptr[i], X.indptr[i + 1]):
                    data[q] /= nv
    elif axis == 0:
        norms = [0.0] * X.d
        for j, val in zip(X.indices, data):
            norms[j] = f(norms[j], val)
        for j in range(X.d):
            norms[j] = g(norms[j])
        for q, j in enumerate(X.indices):
            if norms[j] != 0.0:
                data[q] /= norms[j]
    else:
        raise ValueError("axis must be 0 or 1")
    return Csr(X.indptr, X.indices, data, X.n, X.d, X.fields, X.n_fields, X.y)


_DIGITS = "0123456789"


def _lines(text):
    """Nim's `lines`: split at "\\n", a "\\r" before it dropped, no empty line after a final newline"""
    out = text.split("\n")
    if out and out[-1] == "":
        out.pop()
    return [ln[:-1] if ln.endswith("\r") else ln for ln in out]


def _skip_until_digit(line, start):
    p = start
    while p < len(line) and line[p] not in _DIGITS:
        p += 1
    return p


def _parse_int(line, start):
    p = start
    while p < len(line) and line[p] in _DIGITS:
        p += 1
    return (int(line[start:p]) if p > start else None), p


def _parse_float(line, start):
    """parseutils.parseFloat from a digit: digits [. digits] [e|E [+-] digits]"""
    p = start
    while p < len(line) and line[p] in _DIGITS:
        p += 1
    if p < len(line) and line[p] == ".":
        p += 1
        while p < len(line) and line[p] in _DIGITS:
            p += 1
    if p < len(line) and line[p] in "eE":
        q = p + 1
        if q < len(line) and line[q] in "+-":
            q += 1
        if q < len(line) and line[q] in _DIGITS:
            while q < len(line) and line[q] in _DIGITS:
                q += 1
            p = q
    return (float(line[start:p]) if p > start else None), p


def load_user_item(text):
    """dataset.nim:840-900, character by character.  ValueError where the reference's reading is undefined: a line of
    exactly four characters (counted by :853, skipped by :872), a line with fewer than three numbers, no line at all."""
    users, items, y = [], [], []
    min_user, max_user, min_item, max_item = 1, 0, 1, 0
    for no, line in enumerate(_lines(text)):
        if len(line) < 4:
            continue
        if len(line) < 5:
            raise ValueError("line %d has exactly four characters" % (no + 1))
        u, p = _parse_int(line, _skip_until_digit(line, 0))
        it, p = (None, p) if u is None else _parse_int(line, _skip_until_digit(line, p))
        r, p = (None, p) if it is None else _parse_float(line, _skip_until_digit(line, p))
        if r is None:
            raise ValueError("line %d has fewer than three numbers" % (no + 1))
        users.append(u)
        items.append(it)
        y.append(r)
        min_user, max_user = min(min_user, u), max(max_user, u)
        min_item, max_item = min(min_item, it), max(max_item, it)
    if not y:
        raise ValueError("no line")
    n_users, n_items = max_user - min_user + 1, max_item - min_item + 1
    indices = []
    for u, it in zip(users, items):
        indices += [u - min_user, it + n_users - min_item]
    n = len(y)
    return Csr([2 * i for i in range(n + 1)], indices, [1.0] * (2 * n), n, n_users + n_items, y=y)
