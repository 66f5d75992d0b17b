"""Plain-Python restatement of the reference's column-major dataset procs, loop for loop in its order, for the device
versions (nimfm_amd/csrc/dataset_csc.hip) to be compared with bit for bit:

    toCSCMatrix / toCSRMatrix         tensor/sparse.nim:510-527 / :490-507
    X[a..<b] of a CSCMatrix           tensor/sparse.nim:300-325
    vstack / hstack of CSCMatrices    tensor/sparse.nim:583-610 / :701-716
    normalize of a ColMatrix          tensor/sparse.nim:414-427 (the generic fold of :372-394 with 1 - axis)
    loadUserItemRatingFile as CSC     dataset.nim:903-992
    decisionFunction of a ColDataset  kernels.nim:4-44 (the order of a sample's terms only: ascending column id)

Every array is a copy, an integer or an in-order fold.  Nothing is vectorised: the order of every sum is the order of the
loop.  Written from the cited lines, not copied from them.
"""
from dataset_ops_restatement import NORMS, Csr, _lines, _parse_float, _parse_int, _skip_until_digit, check_indices_row


class Csc:
    """CSCMatrix (tensor/sparse.nim:14-17) with the targets the device dataset carries along: indptr has d + 1 entries,
    indices are sample ids"""

    def __init__(self, indptr, indices, data, n, d, y=None):
        self.indptr, self.indices, self.data = [int(v) for v in indptr], [int(v) for v in indices], [float(v) for v in data]
        self.n, self.d = int(n), int(d)
        self.y = None if y is None else [float(v) for v in y]

    @property
    def nnz(self):
        return len(self.data)

    def dense(self):
        """the last entry of a repeated (i, j) wins, as in Csr.dense"""
        out = [[0.0] * self.d for _ in range(self.n)]
        for j in range(self.d):
            for q in range(self.indptr[j], self.indptr[j + 1]):
                out[self.indices[q]][j] = self.data[q]
        return out


def _cumsum(a):
    for i in range(1, len(a)):
        a[i] += a[i - 1]


def to_csc(X):
    """tensor/sparse.nim:510-527"""
    data, indices, indptr = [0.0] * X.nnz, [0] * X.nnz, [0] * (X.d + 1)
    for i in range(X.n):
        for q in range(X.indptr[i], X.indptr[i + 1]):
            indptr[X.indices[q] + 1] += 1
    _cumsum(indptr)
    offsets = [0] * X.d
    for i in range(X.n):
        for q in range(X.indptr[i], X.indptr[i + 1]):
            j = X.indices[q]
            data[indptr[j] + offsets[j]] = X.data[q]
            indices[indptr[j] + offsets[j]] = i
            offsets[j] += 1
    return Csc(indptr, indices, data, X.n, X.d, X.y)


def to_csr(X):
    """tensor/sparse.nim:490-507"""
    data, indices, indptr = [0.0] * X.nnz, [0] * X.nnz, [0] * (X.n + 1)
    for j in range(X.d):
        for q in range(X.indptr[j], X.indptr[j + 1]):
            indptr[X.indices[q] + 1] += 1
    _cumsum(indptr)
    offsets = [0] * X.n
    for j in range(X.d):
        for q in range(X.indptr[j], X.indptr[j + 1]):
            i = X.indices[q]
            data[indptr[i] + offsets[i]] = X.data[q]
            indices[indptr[i] + offsets[i]] = j
            offsets[i] += 1
    return Csr(indptr, indices, data, X.n, X.d, y=X.y)


def slice_rows(X, a, b):
    """X[a..<b] = X[a..b-1], tensor/sparse.nim:300-325; the targets are sliced"""
    check_indices_row(X, list(range(a, b)))
    lo, hi = a, b - 1
    indptr = [0] * (X.d + 1)
    for j in range(X.d):
        for q in range(X.indptr[j], X.indptr[j + 1]):
            if lo <= X.indices[q] <= hi:
                indptr[j + 1] += 1
    _cumsum(indptr)
    nnz = indptr[-1]
    indices, data = [0] * nnz, [0.0] * nnz
    for j in range(X.d):
        count = 0
        for q in range(X.indptr[j], X.indptr[j + 1]):
            if lo <= X.indices[q] <= hi:
                indices[indptr[j] + count] = X.indices[q] - lo
                data[indptr[j] + count] = X.data[q]
                count += 1
    return Csc(indptr, indices, data, hi - lo + 1, X.d, None if X.y is None else X.y[a:b])


def vstack(parts, reference_indptr_length=False):
    """tensor/sparse.nim:583-610.  reference_indptr_length: size the result's indptr by shape[0] + 1 as :598 does -- an
    IndexError with fewer rows than columns, a tail nothing reads with more; the device (and the default here) sizes it by
    shape[1] + 1, the one departure of DESIGN.md section 25."""
    first = parts[0]
    n, d = first.n, first.d
    for X in parts[1:]:
        if X.d != d:
            raise ValueError("All matrics must have the same shape[1].")
        n += X.n
    indptr = [0] * ((n if reference_indptr_length else d) + 1)
    data, indices = [], []
    for j in range(d):
        offset = 0
        for X in parts:
            for q in range(X.indptr[j], X.indptr[j + 1]):
                data.append(X.data[q])
                indices.append(X.indices[q] + offset)
                indptr[j + 1] += 1
            offset += X.n
    _cumsum(indptr)
    y = [v for X in parts for v in X.y] if all(X.y is not None for X in parts) else None
    return Csc(indptr, indices, data, n, d, y)


def hstack(parts):
    """tensor/sparse.nim:701-716; the targets of the first part, as the row-major hstack keeps them"""
    first = parts[0]
    indptr, indices, data, d = list(first.indptr), list(first.indices), list(first.data), first.d
    for X in parts[1:]:
        nnz = len(data)
        if X.n != first.n:
            raise ValueError("All matrics must have the same shape[0]")
        data += X.data
        indices += X.indices
        indptr += [nnz + v for v in X.indptr[1:]]
        d += X.d
    return Csc(indptr, indices, data, first.n, d, first.y)


def normalize(X, axis, norm):
    """tensor/sparse.nim:414-427 into a copy: the generic fold (:372-394) called with 1 - axis, nRows = shape[1] and
    nCols = shape[0] on the column arrays"""
    f, g = NORMS[norm]
    data = list(X.data)
    t_axis, n_rows, n_cols = 1 - axis, X.d, X.n
    if t_axis == 1:  # axis 0: along each column's segment
        for i in range(n_rows):
            nv = 0.0
            for q in range(X.indptr[i], X.indptr[i + 1]):
                nv = f(nv, data[q])
            nv = g(nv)
            if nv != 0.0:
                for q in range(X.indptr[i], X.indptr[i + 1]):
                    data[q] /= nv
    elif t_axis == 0:  # axis 1: a sample's entries in column-major storage position
        norms = [0.0] * n_cols
        for j, val in zip(X.indices, data):
            norms[j] = f(norms[j], val)
        for j in range(n_cols):
            norms[j] = g(norms[j])
        for q, j in enumerate(X.indices):
            if norms[j] != 0.0:
                data[q] /= norms[j]
    else:
        raise ValueError("axis must be 0 or 1")
    return Csc(X.indptr, X.indices, data, X.n, X.d, X.y)


def load_user_item_csc(text):
    """dataset.nim:903-992, three passes; every pass skips lines of fewer than FIVE characters (:923, 955, 975), so a
    four-character line is skipped.  ValueError where the reading is undefined: a line with fewer than three numbers, no
    line at all (as the row-major loader's restatement)."""
    kept = []
    min_user, max_user, min_item, max_item = 1, 0, 1, 0
    for no, line in enumerate(_lines(text)):
        if len(line) < 5:
            continue
        u, p = _parse_int(line, _skip_until_digit(line, 0))
        it, p = (None, p) if u is None else _parse_int(line, _skip_until_digit(line, p))
        r, p = (None, p) if it is None else _parse_float(line, _skip_until_digit(line, p))
        if r is None:
            raise ValueError("line %d has fewer than three numbers" % (no + 1))
        kept.append((u, it, r))
        min_user, max_user = min(min_user, u), max(max_user, u)
        min_item, max_item = min(min_item, it), max(max_item, it)
    if not kept:
        raise ValueError("no line")
    n_users, n_items = max_user - min_user + 1, max_item - min_item + 1
    d, n = n_users + n_items, len(kept)
    indptr = [0] * (d + 1)
    for u, it, _ in kept:
        indptr[u - min_user + 1] += 1
        indptr[it - min_item + n_users + 1] += 1
    _cumsum(indptr)
    indices, offsets = [0] * (2 * n), [0] * d
    for i, (u, it, _) in enumerate(kept):
        for j in (u - min_user, it - min_item + n_users):
            indices[indptr[j] + offsets[j]] = i
            offsets[j] += 1
    return Csc(indptr, indices, [1.0] * (2 * n), n, d, [r for _, _, r in kept])


def column_walk_order(X):
    """per sample the (column, value) terms in the order a column walk meets them (kernels.nim:4-44: `for j in 0..<nFeatures:
    for (i, val) in X.getCol(j)`): ascending j, repeats in column-storage order -- the storage order of to_csr(X)"""
    terms = [[] for _ in range(X.n)]
    for j in range(X.d):
        for q in range(X.indptr[j], X.indptr[j + 1]):
            terms[X.indices[q]].append((j, X.data[q]))
    return terms
