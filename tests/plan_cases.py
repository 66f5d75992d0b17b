"""Inputs for the batch-plan tests, shared by tests/test_plan_restatement.py (CPU: every case has the property its name
claims) and tests/test_gpu_plan.py (every build of every case equals tests/plan_restatement.py, array for array).

A CASE is one dataset (built from fixed seeds, cached) and a list of BUILDS on it, in order: the dataset's state (its
column-major twin, "a cell overflowed once") carries from one build to the next, which some cases are about.  A build
names the plan's arguments, the environment knobs, the flag combinations to run, what the plan must say about who built
it (`expect`, asserted against the read-back, never assumed) and what the data must be like for the name to be true
(`claims`, asserted on the CPU from the data alone).

Everything here is sized for seconds: plans need no model, so d is free; rows stay at or below a few tens of thousands.
"""
import functools
import itertools

import numpy as np

import plan_route_cases as PR

I64 = np.int64
SORT_ENV = {"NFM_PLAN_SEG": "0", "NFM_PLAN_CSC": "0"}
KNOBS = ("NFM_PLAN_SEG", "NFM_PLAN_CSC", "NFM_PLAN_KEY", "NFM_SEG_FL", "NFM_SEG_S", "NFM_SEG_XCD")

FLAG_NAMES = ("first_singleton", "want_tq", "use_singles", "sort_by_count")
ALL8 = [dict(zip(("want_tq", "use_singles", "sort_by_count"), v)) for v in itertools.product((False, True), repeat=3)]
PLAIN = [dict()]
TWIN_FLAGS = [dict(), dict(sort_by_count=True, want_tq=True)]
SEG_FLAGS = [dict(), dict(use_singles=True, sort_by_count=True), dict(want_tq=True, use_singles=True),
             dict(sort_by_count=True, want_tq=True)]


class Data:
    def __init__(self, indptr, indices, data, n, d):
        self.indptr, self.indices, self.data = np.asarray(indptr, dtype=I64), np.asarray(indices, dtype=I64), np.asarray(data, dtype=np.float64)
        self.n, self.d = int(n), int(d)
        assert len(self.indptr) == n + 1 and self.indptr[-1] == len(self.indices) == len(self.data)
        assert len(self.indices) == 0 or (self.indices.min() >= 0 and self.indices.max() < d)


class Build:
    def __init__(self, tag, batch, begin=0, end=None, order=("none",), n_aug=0, first_singleton=False, env=None, flags=PLAIN,
                 expect=None, claims=None, versus_sort=False):
        self.tag, self.batch, self.begin, self.end, self.order, self.n_aug = tag, batch, begin, end, order, n_aug
        self.first_singleton, self.env, self.flags = first_singleton, dict(env or {}), flags
        self.expect, self.claims, self.versus_sort = dict(expect or {}), dict(claims or {}), versus_sort


class Case:
    def __init__(self, name, make, builds):
        self.name, self._make, self.builds = name, make, builds

    @functools.lru_cache(maxsize=None)
    def data(self):
        return self._make()


# ---------------------------------------------------------------- generators
def _values(nnz, seed):
    v = np.random.default_rng(seed).uniform(0.25, 1.75, size=nnz)
    v[::3] *= -1.0
    return v


def from_pairs(rows, cols, n, d, seed, unsorted=False):
    """CSR of the (row, column) pairs, ascending inside a row; unsorted: every odd row stored in descending order"""
    rows, cols = np.asarray(rows, dtype=I64), np.asarray(cols, dtype=I64)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    assert len(rows) == 0 or not ((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])).any(), "a row repeats a column"
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(I64)
    if unsorted and len(rows):
        m = np.diff(indptr)[rows]
        within = np.arange(len(rows)) - indptr[rows]
        flip = rows % 2 == 1
        src = np.where(flip, indptr[rows] + m - 1 - within, np.arange(len(rows)))
        cols = cols[src]
    return Data(indptr, cols, _values(len(cols), seed), n, d)


def strided_rows(lens, d, seed, unsorted=False):
    """row i: lens[i] distinct features start_i + step * (0 .. len-1) mod d (step odd for a power of two d, else 1)"""
    lens = np.asarray(lens, dtype=I64)
    n = len(lens)
    rng = np.random.default_rng(seed)
    assert lens.max(initial=0) <= d
    start = rng.integers(0, d, size=n)
    pow2 = d & (d - 1) == 0
    step = rng.integers(0, 8, size=n) * 2 + 1 if pow2 else np.ones(n, dtype=I64)
    rows = np.repeat(np.arange(n), lens)
    within = np.arange(lens.sum()) - np.repeat(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    cols = (start[rows] + step[rows] * within) % d
    return from_pairs(rows, cols, n, d, seed + 1, unsorted)


def column_lengths(n, d, collens, seed, unsorted=False):
    """column j is stored in exactly collens[j] rows (column 0 in the first ones, the others in random ones)"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j, L in enumerate(collens):
        assert L <= n
        r = np.arange(L) if j == 0 else np.sort(rng.permutation(n)[:L])
        rows.append(r)
        cols.append(np.full(L, j))
    return from_pairs(np.concatenate(rows), np.concatenate(cols), n, d, seed + 1, unsorted)


def cells(batch_rows, d, fl, counts, seed, mult=5, spread=256):
    """Exact (batch, bucket) cells: batch b has batch_rows[b] rows and counts[b][k] touches in bucket k (features
    k 2^fl ...).  Touch i of a cell goes to row i mod rows and feature offset (i div rows + mult (i mod rows)) mod
    min(width, spread): distinct inside a row, repeated across rows."""
    rows_all, cols_all, r0 = [], [], 0
    for b, B in enumerate(batch_rows):
        for k, c in enumerate(counts[b]):
            if c == 0:
                continue
            width = min(1 << fl, d - (k << fl), spread)
            assert width > 0 and -(-c // B) <= width
            i = np.arange(c, dtype=I64)
            rows_all.append(r0 + i % B)
            cols_all.append((k << fl) + (i // B + mult * (i % B)) % width)
        r0 += B
    return from_pairs(np.concatenate(rows_all), np.concatenate(cols_all), r0, d, seed)


def within_batches_perm(n, batch, seed):
    """a host order that keeps every batch's set of samples: position p holds a sample of p's own batch"""
    rng = np.random.default_rng(seed)
    return np.concatenate([s + rng.permutation(min(batch, n - s)) for s in range(0, n, batch)]).astype(I64)


# ---------------------------------------------------------------- properties, computed from the data alone
def resolve_order(build, data, device_perm=None):
    kind = build.order[0]
    if kind == "none":
        return None
    if kind == "host":
        return np.asarray(build.order[1], dtype=I64)
    full = np.zeros(build.end if build.end is not None else data.n, dtype=I64)  # device: the read-back, placed at [begin, end)
    full[build.begin:] = device_perm
    return full


def range_of(build, data):
    end = data.n if build.end is None else build.end
    return build.begin, end


def touch_table(data, build, perm):
    """(batch, feature) of every stored entry of the range, in sample order (no dummies)"""
    from plan_restatement import batch_bounds
    begin, end = range_of(build, data)
    ns = end - begin
    samp = perm[begin:end] if perm is not None else begin + np.arange(ns)
    m = data.indptr[samp + 1] - data.indptr[samp]
    bp = batch_bounds(ns, build.batch, build.first_singleton)
    pos = np.repeat(np.arange(ns), m)
    start = np.repeat(np.concatenate([[0], np.cumsum(m)[:-1]]) if ns else np.zeros(0, dtype=I64), m)
    src = data.indptr[samp[pos]] + (np.arange(m.sum()) - start)
    b = np.searchsorted(bp, pos, side="right") - 1
    return b, data.indices[src].astype(I64), bp, m


def largest_cell(data, build, perm, fl):
    b, f, bp, _ = touch_table(data, build, perm)
    nbk = ((data.d - 1) >> fl) + 1
    return int(np.bincount(b * nbk + (f >> fl)).max())


def touch_counts(data, build, perm):
    """sorted multiset of touches per (batch, feature)"""
    b, f, bp, _ = touch_table(data, build, perm)
    return np.unique(b * I64(data.d) + f, return_counts=True)[1]


# the bit sums and the bucket width of a build's data, by the route's restatement (tests/plan_route_cases.py)
def key_bit_sum(data, build):
    """fbits + bbits as the sort's key is sized: features d + n_aug, batches ceil(ns / batch) + 1"""
    begin, end = range_of(build, data)
    return PR.key_bit_sum(data.d, build.n_aug, end - begin, build.batch)


def item_bit_sum(data, build, fl):
    from plan_restatement import batch_bounds
    begin, end = range_of(build, data)
    bp = batch_bounds(end - begin, build.batch, build.first_singleton)
    return PR.item_bit_sum(fl, int(np.diff(bp).max()), int(np.diff(data.indptr).max()))


def natural_fl(data, build, perm):
    """the bucket width bucketing chooses by itself, from the build's touches per batch"""
    b, f, bp, m = touch_table(data, build, perm)
    return PR.natural_fl(data.d, m.sum() / (len(bp) - 1))


# ---------------------------------------------------------------- the sort path
def _sort(tag, batch, **kw):
    kw.setdefault("env", SORT_ENV)
    kw.setdefault("expect", {})
    kw["expect"].setdefault("builder", "sort")
    return Build(tag, batch, **kw)


def _ragged():
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 41, size=300)
    lens[3::7] = 0
    lens[11] = 50
    return strided_rows(lens, 50, 6, unsorted=True)


_PERM300 = np.random.default_rng(7).permutation(300)
_STREAM = np.random.default_rng(8).integers(0, 300, size=700)


def _gaps():  # 6 batches of 10; the rows of batches 0, 3 and 5 are empty
    lens = np.full(60, 6)
    for b in (0, 3, 5):
        lens[b * 10:(b + 1) * 10] = 0
    return strided_rows(lens, 16, 9)


def _all_singles():  # batch 1 (rows 10..19): ten rows of three features, no feature twice; the other batches repeat features
    rows = np.repeat(np.arange(40), 3)
    cols = np.where((rows >= 10) & (rows < 20), (rows - 10) * 3 + np.tile(np.arange(3), 40), (rows % 4) + 2 * np.tile(np.arange(3), 40))
    return from_pairs(rows, cols, 40, 32, 10)


def _one_per_row(n, d, seed):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, d, size=n)
    cols[0], cols[-1] = d - 1, 0
    return from_pairs(np.arange(n), cols, n, d, seed)


def _exact_counts():  # one batch of 24 rows: feature j is in exactly j rows, j = 1 .. 20
    rows = np.concatenate([np.arange(j) for j in range(1, 21)])
    cols = np.concatenate([np.full(j, j) for j in range(1, 21)])
    return from_pairs(rows, cols, 24, 24, 12)


_HEAVY_COUNTS = [[128, 129, 192, 193, 300], [129, 128, 193, 192, 257]]


def _heavy_edges():  # batches of 320 and 310 rows: feature j is in the first _HEAVY_COUNTS[b][j] rows of batch b
    rows, cols = [], []
    for b, cs in enumerate(_HEAVY_COUNTS):
        for j, c in enumerate(cs):
            rows.append(b * 320 + np.arange(c))
            cols.append(np.full(c, j))
    return from_pairs(np.concatenate(rows), np.concatenate(cols), 630, 7, 13)


def _heavy_plateaus():  # 5 batches of 140 rows; feature 0 in every row of batches 0, 2 and 4, feature 1 + (row mod 3) everywhere
    r = np.arange(700)
    on = ((r // 140) % 2 == 0)
    return from_pairs(np.concatenate([r[on], r]), np.concatenate([np.zeros(on.sum(), dtype=I64), 1 + r % 3]), 700, 6, 14)


def _dummies():
    return strided_rows(np.random.default_rng(15).integers(0, 5, size=300), 40, 16)


SORT_CASES = [
    Case("sort_ragged", _ragged, [
        _sort("own order, every flag", 32, flags=ALL8),
        _sort("host order, every flag", 32, order=("host", _PERM300), flags=ALL8),
        _sort("sub-range", 32, begin=17, end=263, flags=SEG_FLAGS),
        _sort("sub-range, host order", 32, begin=17, end=263, order=("host", _PERM300), flags=SEG_FLAGS),
        _sort("first singleton", 32, first_singleton=True, flags=SEG_FLAGS),
        _sort("index stream past the end of the data", 50, begin=20, end=700, order=("host", _STREAM), flags=SEG_FLAGS),
        _sort("ns = 0", 16, begin=5, end=5, flags=SEG_FLAGS),
        _sort("ns = 0, host order", 16, begin=5, end=5, order=("host", _PERM300)),
        _sort("ns = 1", 16, begin=5, end=6, flags=SEG_FLAGS),
        _sort("ns = 1 on an empty row (no touch at all)", 16, begin=3, end=4, flags=SEG_FLAGS),
        _sort("ns = batch", 16, begin=5, end=21),
        _sort("ns = batch + 1", 16, begin=5, end=22),
        _sort("first singleton, ns = 1", 16, begin=5, end=6, first_singleton=True),
        _sort("first singleton, ns = 1 + 2 batch", 16, begin=5, end=38, first_singleton=True),
        _sort("batch > ns", 301, flags=SEG_FLAGS, expect=dict(n_batches=1)),
        _sort("batch = 2^32 + 7", 2**32 + 7, flags=SEG_FLAGS, expect=dict(n_batches=1)),
        _sort("batch = 2^32", 2**32, expect=dict(n_batches=1)),
        _sort("batch = 2^63 - 1, first singleton", 2**63 - 1, first_singleton=True, expect=dict(n_batches=2)),
    ]),
    Case("sort_untouched_batches", _gaps, [
        _sort("batches 0, 3, 5 without a touch", 10, flags=ALL8, claims=dict(empty_batches=[0, 3, 5])),
    ]),
    Case("sort_all_singles_batch", _all_singles, [
        _sort("batch 1 is singles only", 10, flags=ALL8, claims=dict(single_only_batch=1)),
    ]),
    Case("sort_key32", lambda: _one_per_row(4095, 2**20, 17), [
        _sort("20 + 12 bits", 1, flags=[dict(), dict(use_singles=True)], expect=dict(key_bits=32), claims=dict(key_sum=32)),
    ]),
    Case("sort_key33", lambda: _one_per_row(4096, 2**20, 18), [
        _sort("20 + 13 bits", 1, flags=[dict(), dict(sort_by_count=True, want_tq=True)], expect=dict(key_bits=64), claims=dict(key_sum=33)),
        _sort("20 + 1 bits", 4096, flags=[dict(sort_by_count=True)], expect=dict(key_bits=32), claims=dict(key_sum=21)),
    ]),
    Case("sort_key_d_2p21", lambda: strided_rows(np.random.default_rng(19).integers(0, 4, size=2000), 2**21 + 3, 20), [
        _sort("22 + 11 bits", 1, expect=dict(key_bits=64), claims=dict(key_sum=33)),
        _sort("22 + 5 bits", 100, flags=SEG_FLAGS, expect=dict(key_bits=32), claims=dict(key_sum=27)),
    ]),
    Case("sort_dummies_heavy", _dummies, [
        _sort("n_aug = 1, batch 150", 150, n_aug=1, flags=ALL8, claims=dict(dummy_touches=150)),
        _sort("n_aug = 2, batch 150, host order", 150, n_aug=2, order=("host", _PERM300), flags=SEG_FLAGS, claims=dict(dummy_touches=150)),
    ]),
    Case("sort_exact_counts", _exact_counts, [
        _sort("counts 1 .. 20", 24, flags=ALL8, claims=dict(counts=list(range(1, 21)))),
    ]),
    Case("sort_heavy_edges", _heavy_edges, [
        _sort("128 129 192 193 300 | 129 128 193 192 257", 320, flags=ALL8, claims=dict(counts=sorted(sum(_HEAVY_COUNTS, [])))),
    ]),
    Case("sort_heavy_plateaus", _heavy_plateaus, [
        _sort("heavy in batches 0, 2, 4", 140, flags=SEG_FLAGS, claims=dict(heavy_batches=[0, 2, 4])),
    ]),
]


# ---------------------------------------------------------------- the column-major twin
def _twin(tag, batch, ne, by_key=0, **kw):
    kw.setdefault("flags", TWIN_FLAGS)
    kw["expect"] = dict(builder="twin", csc_ne=ne, csc_by_key=by_key, **kw.get("expect", {}))
    return Build(tag, batch, versus_sort=True, **kw)


def _longest(L):
    return lambda: column_lengths(L + 40, 6, [L] + [L // 2 + 7 * j for j in range(1, 6)], 30 + L % 17)


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(I64)


def _longest_case(L, ne):
    n = L + 40
    return Case("twin_longest_%d" % L, _longest(L), [
        _twin("NE = %d" % ne, 100, ne, order=("host", _perm(n, L)), claims=dict(max_col=L)),
    ])


def _d37():  # 200 rows, 37 columns (a tail group of one column, a tail workgroup), columns 5 and 36 empty, stored unsorted
    rng = np.random.default_rng(31)
    M = rng.random((200, 37)) < 0.6
    M[:, 5] = False
    M[:, 36] = False
    r, c = np.nonzero(M)
    return from_pairs(r, c, 200, 37, 32, unsorted=True)


def _outside():  # 300 rows, 12 columns; columns 0 and 1 only in rows >= 200, which the order keeps out of [40, 140)
    rng = np.random.default_rng(33)
    M = rng.random((300, 12)) < 0.85
    M[:200, :2] = False
    M[200:, 2:4] = False
    r, c = np.nonzero(M)
    return from_pairs(r, c, 300, 12, 34)


_OUT_PERM = np.concatenate([200 + np.arange(40), _perm(200, 35), 240 + np.arange(60)]).astype(I64)  # positions 40..239 hold rows < 200


def _dense8(n, seed):  # every row has 6 of 8 columns
    rng = np.random.default_rng(seed)
    drop = rng.integers(0, 8, size=n)
    M = np.ones((n, 8), dtype=bool)
    M[np.arange(n), drop] = False
    M[np.arange(n), (drop + 1 + rng.integers(0, 7, size=n)) % 8] = False
    r, c = np.nonzero(M)
    return from_pairs(r, c, n, 8, seed + 1)


def _three_of_8(n, seed):  # row r has columns r, r + 3 and r + 5 mod 8: every column in 3 n / 8 rows
    rows = np.repeat(np.arange(n), 3)
    return from_pairs(rows, (rows + np.tile([0, 3, 5], n)) % 8, n, 8, seed)


def _every_row():  # 400 rows, 10 columns, column 0 in every row: 200 touches in a batch of 200
    rng = np.random.default_rng(37)
    M = rng.random((400, 10)) < 0.6
    M[:, 0] = True
    r, c = np.nonzero(M)
    return from_pairs(r, c, 400, 10, 38)


_REPEAT = _perm(200, 39)
_REPEAT[17] = _REPEAT[3]

_DEV_RANGES = [(0, 1), (0, 2), (0, 3), (0, 1000), (0, 1025), (100, 900)]


def _device_builds():
    out = []
    for (a, b) in _DEV_RANGES:
        for key_env, by_key in (({}, 1), ({"NFM_PLAN_KEY": "0"}, 0)):
            out.append(_twin("drawn order [%d, %d)%s" % (a, b, " from the table" if not by_key else ""), 128, 16, by_key, begin=a, end=b,
                             order=("device", (4242 + b, 3)), env=key_env, flags=[dict(sort_by_count=True, want_tq=True)],
                             claims=dict(max_col_in=(513, 1024))))
    return out


TWIN_CASES = [
    _longest_case(256, 4), _longest_case(257, 8), _longest_case(512, 8), _longest_case(513, 16), _longest_case(1024, 16),
    Case("twin_longest_1025", _longest(1025), [
        Build("not the twin", 300, order=("host", _perm(1065, 1025)), flags=TWIN_FLAGS,
              expect=dict(builder="sort", csc_built=1, csc_usable=0, csc_max_col=1025), claims=dict(max_col=1025)),
        Build("and not on the next build", 500, order=("host", _perm(1065, 1026)), expect=dict(builder="sort", csc_built=1, csc_usable=0)),
    ]),
    Case("twin_d37", _d37, [
        _twin("7 batches", 32, 4, order=("host", _perm(200, 40)), flags=[dict(), dict(want_tq=True), dict(sort_by_count=True, want_tq=True)],
              claims=dict(empty_columns=[5, 36], unsorted=True)),
        _twin("first singleton", 32, 4, order=("host", _perm(200, 41)), first_singleton=True),
        _twin("one batch", 200, 4, order=("host", _perm(200, 42)), expect=dict(n_batches=1)),
        _twin("batch = 2^32 + 7", 2**32 + 7, 4, order=("host", _perm(200, 43)), expect=dict(n_batches=1)),
        _twin("batch = 2^32", 2**32, 4, order=("host", _perm(200, 44)), first_singleton=True, expect=dict(n_batches=2)),
        Build("an order with one sample twice", 32, order=("host", _REPEAT), flags=TWIN_FLAGS, expect=dict(builder="sort"),
              claims=dict(repeats=True)),
    ]),
    Case("twin_columns_outside", _outside, [
        _twin("sub-range [40, 140)", 25, 8, begin=40, end=140, order=("host", _OUT_PERM), claims=dict(columns_outside=[0, 1])),
    ]),
    Case("twin_batch_counts", lambda: _dense8(1026, 45), [
        _twin("64 batches", 16, 16, end=1024, order=("host", _perm(1026, 46)), expect=dict(n_batches=64)),
        _twin("65 batches", 16, 16, end=1025, order=("host", _perm(1026, 47)), expect=dict(n_batches=65)),
        _twin("512 batches", 2, 16, end=1024, order=("host", _perm(1026, 48)), expect=dict(n_batches=512)),
        Build("513 batches", 2, order=("host", _perm(1026, 49)), flags=TWIN_FLAGS, expect=dict(builder="sort", n_batches=513)),
    ]),
    # 8 entries per lane of k_csc_fill at 511 and 512 batches: four wavefronts per workgroup hold 48 KB of LDS at 511, and would
    # ask for 49184 bytes at 512, where twin_fill (plan_route.h) launches two
    Case("twin_batch_counts_ne8", lambda: _three_of_8(1026, 58), [
        _twin("511 batches", 2, 8, end=1022, order=("host", _perm(1026, 59)), expect=dict(n_batches=511), claims=dict(max_col_in=(257, 512))),
        _twin("512 batches", 2, 8, end=1024, order=("host", _perm(1026, 60)), expect=dict(n_batches=512), claims=dict(max_col_in=(257, 512))),
    ]),
    Case("twin_heavy", _every_row, [
        _twin("a column in every row of a batch of 200", 200, 8, order=("host", _perm(400, 50)), claims=dict(counts_max=200)),
    ]),
    Case("twin_device_orders", lambda: _dense8(1025, 51), _device_builds()),
    Case("twin_fill_passes", lambda: strided_rows(np.full(40, 600), 20000, 52), [
        _twin("d = 20000, two batches", 20, 4, order=("host", _perm(40, 53)), flags=[dict(sort_by_count=True, want_tq=True)],
              claims=dict(dense=True)),
    ]),
    Case("twin_count_passes", lambda: strided_rows(np.full(40, 1000), 70000, 54), [
        _twin("d = 70000, one batch", 40, 4, order=("host", _perm(40, 55)), flags=[dict()], claims=dict(dense=True)),
    ]),
    Case("twin_units_passes", lambda: strided_rows(np.full(248, 4500), 70000, 56), [
        _twin("d = 70000, 31 batches: more cells than one pass of k_csc_units", 8, 4, order=("host", _perm(248, 57)), flags=[dict(want_tq=True)],
              claims=dict(dense=True, cells_above=256 * 32 * 256)),
    ]),
]


# ---------------------------------------------------------------- bucketing
def _seg(tag, batch, fl, bits, ipt, **kw):
    kw.setdefault("flags", SEG_FLAGS)
    kw["expect"] = dict(builder="seg", seg_fl=fl, seg_item_bits=bits, seg_ipt=ipt, **kw.get("expect", {}))
    cl = dict(kw.get("claims", {}))
    cl.setdefault("touches_per_batch_at_least", 8192)
    cl.setdefault("item_sum_fits" if bits == 32 else "item_sum_over", fl)
    kw["claims"] = cl
    return Build(tag, batch, versus_sort=True, **kw)


def _cell_case(M, ipt):
    """d = 65536, two batches of 2048 rows, fl = 12: 16 buckets of 600 touches, but cell (0, 0) of exactly M"""
    counts = [[M] + [600] * 15, [600] * 16]
    make = lambda: cells([2048, 2048], 65536, 12, counts, 60 + M % 13)
    perm = within_batches_perm(4096, 2048, M)
    if M <= 4096:
        builds = [_seg("largest cell %d" % M, 2048, 12, 32, ipt, order=("host", perm), expect=dict(seg_max_cell=M, seg_nbk=16),
                       claims=dict(max_cell=(12, M), natural_fl=12))]
    else:
        # (one flag combination: the overflow is remembered with the dataset, the next build would not try bucketing)
        builds = [Build("largest cell %d: the sort" % M, 2048, order=("host", perm), flags=[dict(use_singles=True, sort_by_count=True, want_tq=True)],
                        expect=dict(builder="sort", seg_max_cell=M, seg_unfit=1), claims=dict(max_cell=(12, M), natural_fl=12)),
                  Build("and the sort from then on, for a range whose cells would fit", 2048, begin=2048, end=4096,
                        order=("host", within_batches_perm(4096, 2048, 5)), flags=[dict(use_singles=True, sort_by_count=True)],
                        expect=dict(builder="sort", seg_max_cell=0, seg_unfit=1),
                        claims=dict(touches_per_batch_at_least=8192, max_cell=(12, 600), natural_fl=12))]
    return Case("seg_cell_%d" % M, make, builds)


def _wide(extra, rows=16384):
    """`rows` rows of one or two entries over d = 53248 (13 buckets at fl = 12), row 0 with `extra` entries"""
    def make():
        rng = np.random.default_rng(70 + extra)
        lens = rng.integers(1, 3, size=rows)
        lens[0] = extra
        return strided_rows(lens, 53248, 71 + extra)
    return make


def _shape_fl(d, per_row, seed, rows=1000):  # two batches of 500 rows
    return lambda: strided_rows(np.full(rows, per_row), d, seed, unsorted=True)


def _rowlens():  # batches of 256 rows of 48 entries, but empty rows among them and rows of 64, 65 and 200 entries
    lens = np.full(256 * 3 + 100, 48)
    lens[5::11] = 0
    lens[[7, 300, 600]] = 64
    lens[[8, 301]] = 65
    lens[[9, 700]] = 200
    return strided_rows(lens, 4096, 80, unsorted=True)


def _singles_cell():
    """d = 65536, fl = 12, one batch of 2048 rows: bucket 5 holds 1500 touches of 1500 different features, the other
    buckets 700 touches of repeated features; feature 3 of bucket 0 in 129 rows"""
    base = cells([2048], 65536, 12, [[700] * 5 + [0] + [700] * 10], 81)
    r5, c5 = np.arange(1500), 5 * 4096 + np.arange(1500) * 2
    free = np.setdiff1d(np.arange(2048), base_rows_with(base, 3))[:129]
    rows = np.concatenate([np.repeat(np.arange(2048), np.diff(base.indptr)), r5, free])
    cols = np.concatenate([base.indices, c5, np.full(len(free), 3)])
    keep = np.ones(len(rows), dtype=bool)
    keep[:len(base.indices)] = base.indices != 3  # feature 3 comes only from the 129 rows added here
    return from_pairs(rows[keep], cols[keep], 2048, 65536, 82)


def base_rows_with(data, feature):
    rows = np.repeat(np.arange(data.n), np.diff(data.indptr))
    return rows[data.indices == feature]


def _nine_batches():
    return strided_rows(np.full(4500, 24), 4096, 83)


SEG_CASES = [
    _cell_case(1024, 4), _cell_case(1025, 8), _cell_case(2048, 8), _cell_case(2049, 16), _cell_case(4096, 16), _cell_case(4097, 0),
    Case("seg_items_32", _wide(64), [
        _seg("12 + 14 + 6 bits", 16384, 12, 32, 16, flags=[dict(), dict(use_singles=True, sort_by_count=True, want_tq=True)],
             claims=dict(item_sum=32, natural_fl=12, max_row=64)),
    ]),
    Case("seg_items_33_row", _wide(65), [
        _seg("12 + 14 + 7 bits: 64-bit items", 16384, 12, 64, 8, flags=SEG_FLAGS, claims=dict(item_sum=33, natural_fl=12, max_row=65)),
        _seg("the same cut by NFM_SEG_FL=8", 16384, 8, 32, 4, env={"NFM_SEG_FL": "8"}, flags=[dict(use_singles=True)], claims=dict(item_sum=29)),
    ]),
    Case("seg_items_33_batch", _wide(64, rows=16385), [
        _seg("12 + 15 + 6 bits: 64-bit items", 16385, 12, 64, 16, flags=[dict(), dict(use_singles=True, sort_by_count=True, want_tq=True)],
             claims=dict(item_sum=33, natural_fl=12, max_batch=16385)),
        _seg("host order, batches of 8193 and 8192", 8193, 12, 32, 8, order=("host", _perm(16385, 72)),
             flags=[dict(want_tq=True, use_singles=True)], claims=dict(natural_fl=12, item_sum=32)),
    ]),
    Case("seg_fl8", _shape_fl(4096, 64, 73), [_seg("fl = 8 by shape", 500, 8, 32, 16, claims=dict(natural_fl=8), expect=dict(seg_nbk=16))]),
    Case("seg_fl9", _shape_fl(4096, 24, 74), [_seg("fl = 9 by shape", 500, 9, 32, 8, claims=dict(natural_fl=9), expect=dict(seg_nbk=8))]),
    Case("seg_fl10", _shape_fl(8192 - 37, 24, 75), [
        _seg("fl = 10 by shape, d no multiple of 2^fl", 500, 10, 32, 8, claims=dict(natural_fl=10, d_ragged=10), expect=dict(seg_nbk=8)),
        _seg("fl = 8 by NFM_SEG_FL", 500, 8, 32, 4, env={"NFM_SEG_FL": "8"}, flags=[dict(use_singles=True, sort_by_count=True)], expect=dict(seg_nbk=32)),
        _seg("fl = 9 by NFM_SEG_FL", 500, 9, 32, 4, env={"NFM_SEG_FL": "9"}, flags=[dict(want_tq=True)], expect=dict(seg_nbk=16)),
        _seg("fl = 11 by NFM_SEG_FL", 500, 11, 32, 16, env={"NFM_SEG_FL": "11"}, flags=[dict(sort_by_count=True)], expect=dict(seg_nbk=4)),
    ]),
    Case("seg_fl11", _shape_fl(16384 - 5, 24, 76), [
        _seg("fl = 11 by shape", 500, 11, 32, 8, claims=dict(natural_fl=11, d_ragged=11), expect=dict(seg_nbk=8)),
        _seg("fl = 12 by NFM_SEG_FL", 500, 12, 32, 16, env={"NFM_SEG_FL": "12"}, flags=[dict(use_singles=True)], expect=dict(seg_nbk=4)),
    ]),
    Case("seg_4096_buckets", lambda: strided_rows(np.full(4096, 3), 2**24, 77), [
        _seg("d = 2^24", 4096, 12, 32, 4, flags=[dict(), dict(use_singles=True, sort_by_count=True)], expect=dict(seg_nbk=4096), claims=dict(natural_fl=12)),
    ]),
    Case("seg_4097_buckets", lambda: strided_rows(np.full(4096, 3), 2**24 + 1, 78), [
        Build("d = 2^24 + 1: the sort", 4096, flags=[dict(use_singles=True, sort_by_count=True)], expect=dict(builder="sort", seg_max_cell=0),
              claims=dict(touches_per_batch_at_least=8192)),
    ]),
    Case("seg_batch_counts", _nine_batches, [
        _seg("%d batches%s%s" % (nb, ", plain workgroup order" if xcd else "", ", chunks of 64" if s else ""), 500, 9, 32, 8, end=500 * nb,
             env=dict(xcd, **s), flags=[dict(use_singles=True, sort_by_count=True, want_tq=True)],
             expect=dict(n_batches=nb, seg_xcd=0 if xcd else 1, seg_s=64 if s else 256))
        for nb in (1, 7, 8, 9) for xcd in ({}, {"NFM_SEG_XCD": "0"}) for s in (({}, {"NFM_SEG_S": "64"}) if nb == 9 else ({},))
    ]),
    Case("seg_row_lengths", _rowlens, [
        _seg("batches of 256, a short last one", 256, 9, 32, 8, expect=dict(n_batches=4), claims=dict(max_row=200, max_batch=256)),
        _seg("batches of 257", 257, 9, 32, 8, flags=[dict(use_singles=True, want_tq=True)], claims=dict(max_batch=257)),
        _seg("first singleton", 400, 9, 32, 16, first_singleton=True, flags=[dict(sort_by_count=True, want_tq=True)]),
        _seg("sub-range, batches of 301", 301, 9, 32, 16, begin=33, end=800, flags=[dict(use_singles=True, sort_by_count=True)]),
    ]),
    Case("seg_singles_cell", _singles_cell, [
        _seg("a cell of singles, a feature of 129 touches", 2048, 12, 32, 8, claims=dict(natural_fl=12, single_cell=5, counts_max=129)),
        _seg("the same under a host order", 2048, 12, 32, 8, order=("host", _perm(2048, 85)), flags=[dict(use_singles=True, sort_by_count=True, want_tq=True)]),
    ]),
]

CASES = SORT_CASES + TWIN_CASES + SEG_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def flags_of(build, fl):
    kw = dict(first_singleton=build.first_singleton, want_tq=False, use_singles=False, sort_by_count=False)
    kw.update(fl)
    return kw
