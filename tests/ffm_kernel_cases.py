"""The inputs shared by tests/test_ffm_kernel_cases.py (CPU) and tests/test_gpu_ffm_kernels.py: field-aware data sets with explicit
row lengths and explicit per-batch touch counts, the table of (k, F, row lengths) cases, and a restatement of what the host
chooses for each of them -- which of the three row kernels of csrc/mb_ffm.hip a mini-batch takes (k_ffm_row_phase,
k_ffm_row_phase_lds<.., 4, false>: one sample per wavefront, <.., 4, true>: one sample per workgroup) and with how much dynamic
LDS, which batches go through k_ffm_heavy_partial / k_ffm_heavy_apply, which through k_ffm_refresh.

run_ffm counts every row-phase launch under "ffm_row_generic", "ffm_row_lds" or "ffm_row_coop" and, with more than 64 KiB of
dynamic LDS, under "ffm_row_lds_big" (nfm_ctx_timing_get): the GPU tests compare those counters with the restatement below, the
CPU tests assert that the table reaches every lane width under every kernel and sits on both sides of every threshold.

Every function that restates host code names the lines it restates."""
import collections
import functools

import numpy as np

kWave = 64
kHeavyTouches, kHeavySegment = 128, 64  # plan.h:69-70
kFtab = 64  # mb_dev.h
LDS_SHARE = 150 * 1024  # mb_ffm_route.h: kFfmLdsShare
LDS_DEFAULT = 64 * 1024  # mb_ffm_route.h: kFfmLdsDefault; above it hipFuncAttributeMaxDynamicSharedMemorySize is raised
N_TRAIN, BATCH, EPOCHS = 300, 77, 2  # batches of 77, 77, 77 and 69; AdaGrad's first epoch: 1, 77, 77, 77, 68
D_TRAIN = 120
N_HUBS = 3  # two of them in every row of two entries or more
SGD_ETA0, ADA_ETA0 = 0.002, 0.01  # the defaults overshoot on long rows: tests/test_gpu_row_slots.py, ADA_ETA0

RowCase = collections.namedtuple("RowCase", "name k F lengths kernel lds_bytes")


# ---------------------------------------------------------------- the host's choices
def lanes_for_k(k):
    """common.h:208-212"""
    half, L = (k + 1) // 2, 1
    while L < half:
        L <<= 1
    return L


def per_wave_bytes(k, F, max_row):
    """mb_ffm_route.h: ffm_row_lds(max(max_row, 1), F, Kp).per_wave (the kernel's own statement of it: k_ffm_row_phase_lds, mb_ffm.hip)"""
    Kp, m_cap = 2 * lanes_for_k(k), max(max_row, 1)
    per_wave = m_cap * F * Kp * 8 + F * 8 + m_cap * 16
    return (per_wave + 15) // 16 * 16


def row_kernel(k, F, max_row):
    """(kernel, dynamic LDS bytes) of every row-phase launch of a fit: mb_ffm_route.h, ffm_row_kernel, with NFM_FFM_LDS
    unset; the launch itself: run_ffm, mb_ffm.hip.  max_row is the data set's, not the batch's."""
    if max_row <= kWave and F <= kWave:
        per_wave = per_wave_bytes(k, F, max_row)
        if per_wave * 4 <= LDS_SHARE:
            return "lds", per_wave * 4
        if per_wave <= LDS_SHARE:
            return "coop", per_wave
    return "generic", 0


FAMILY = {"generic": "ffm_row_generic", "lds": "ffm_row_lds", "coop": "ffm_row_coop"}
BIG = "ffm_row_lds_big"


def batches(n, batch, first_singleton):
    """[(begin, end)] positions of an epoch's mini-batches (plan.hip:1039: AdaGrad's very first step is a batch of its own)"""
    cuts = [0] + ([1] if first_singleton and n > 0 else [])
    while cuts[-1] < n:
        cuts.append(min(cuts[-1] + batch, n))
    return list(zip(cuts[:-1], cuts[1:]))


def fit_batches(n, batch, solver, perms=None, epochs=EPOCHS):
    """[(sample ids of the batch, stored)] of a fit from it = 1; stored: the batch reads the parameters as stored
    (mb_ffm_route.h: ffm_route, first_stored)"""
    out = []
    for e in range(epochs):
        order = np.arange(n) if perms is None else np.asarray(perms[e])
        first = solver == "adagrad" and e == 0
        for b, (lo, hi) in enumerate(batches(n, batch, first)):
            out.append((order[lo:hi], first and b == 0))
    return out


def batch_counts(X, ids):
    """touches per feature in the mini-batch of the samples `ids`"""
    cols = np.concatenate([X.indices[X.indptr[i]:X.indptr[i + 1]] for i in ids] + [np.zeros(0, np.int64)])
    return np.bincount(cols.astype(np.int64), minlength=X.d)


def heavy_batches(X, batch, solver, perms=None):
    """how many mini-batches of a fit have a feature of more than kHeavyTouches touches (plan.hip:175 and 195-197, the launches:
    run_ffm, mb_ffm.hip, where ffm_route gives nH > 0), and the segments of the widest one"""
    n_b, segs = 0, 0
    for ids, _ in fit_batches(X.n, batch, solver, perms):
        c = batch_counts(X, ids)
        if (c > kHeavyTouches).any():
            n_b += 1
            segs = max(segs, int(-(-c.max() // kHeavySegment)))
    return n_b, segs


def refresh_batches(X, batch, solver, perms=None):
    """how many mini-batches of a fit start with k_ffm_refresh: AdaGrad, not the stored first step, touches >= 4 x unique
    features (mb_ffm_route.h: ffm_route, refresh, with NFM_FFM_REFRESH unset)"""
    if solver != "adagrad":
        return 0
    n_r = 0
    for ids, stored in fit_batches(X.n, batch, solver, perms):
        c = batch_counts(X, ids)
        n_r += int(not stored and c.sum() >= 4 * np.count_nonzero(c))
    return n_r


# ---------------------------------------------------------------- data
class FieldCsr:
    def __init__(self, indptr, indices, data, fields, n, d, F):
        self.indptr, self.indices, self.data, self.fields = (np.asarray(indptr, np.int64), np.asarray(indices, np.int64),
                                                             np.asarray(data, np.float64), np.asarray(fields, np.int64))
        self.n, self.d, self.F = n, d, F
        for a in (self.indptr, self.indices, self.data, self.fields):
            a.setflags(write=False)

    def lengths(self):
        return np.diff(self.indptr)

    def row(self, i):
        return self.indices[self.indptr[i]:self.indptr[i + 1]]


def fields_of(d, F, rng):
    """a field per feature, every field present"""
    assert d >= F
    field_of = rng.integers(0, F, size=d)
    field_of[rng.permutation(d)[:F]] = np.arange(F)
    return field_of


def lengths_ffm(lengths, n, d, F, seed, hubs=N_HUBS):
    """n rows, row i of lengths[i % len(lengths)] entries -- lengths[0] is the longest, so row 0 is (AdaGrad's parameters are a
    function of its state, which starts at zero, and only its first step, a mini-batch of one sample, reads the stored ones:
    tests/row_slot_cases.py, lengths_csr) -- with distinct column ids, two of them from the first `hubs` ids in every row of
    two entries or more, and values from U(-1, 1); every other row (the odd ones) is stored unsorted.  The field is the
    feature's."""
    assert lengths[0] == max(lengths)
    rng = np.random.default_rng(seed)
    field_of = fields_of(d, F, rng)
    rows, vals, indptr = [], [], [0]
    for i in range(n):
        m = lengths[i % len(lengths)]
        if m >= 2:
            idx = np.sort(np.concatenate([rng.choice(hubs, size=2, replace=False), hubs + rng.choice(d - hubs, size=m - 2, replace=False)]))
        else:
            idx = hubs + rng.choice(d - hubs, size=m, replace=False)
        if i % 2 and m >= 2:
            idx = rng.permutation(idx)
            if np.all(np.diff(idx) > 0):
                idx = idx[::-1]
        rows.append(idx.astype(np.int64))
        vals.append(rng.uniform(-1, 1, size=m))
        indptr.append(indptr[-1] + m)
    idx = np.concatenate(rows)
    return FieldCsr(indptr, idx, np.concatenate(vals), field_of[idx], n, d, F)


def with_one_more_row(X, m, seed=65):
    """X and one row of m entries behind it (the fields: the features' own, 0 for a feature X does not have)"""
    rng = np.random.default_rng(seed)
    field_of = np.zeros(X.d, np.int64)
    field_of[X.indices] = X.fields
    idx = rng.permutation(X.d)[:m].astype(np.int64)
    return FieldCsr(np.append(X.indptr, X.indptr[-1] + m), np.concatenate([X.indices, idx]),
                    np.concatenate([X.data, rng.uniform(-1, 1, size=m)]), np.concatenate([X.fields, field_of[idx]]), X.n + 1, X.d, X.F)


def targets(n, seed):
    y = np.random.default_rng(seed).standard_normal(n)
    y.setflags(write=False)
    return y


def start(d, F, k, fit_linear=True):
    """P0 (reference layout [F][d][k]) at scale 0.1 / sqrt(k), w0, b0"""
    rng = np.random.default_rng(k)
    P0 = rng.standard_normal((F, d, k)) * (0.1 / np.sqrt(k))
    w0 = rng.uniform(-0.1, 0.1, d) if fit_linear else np.zeros(d)
    return P0, w0, 0.05


# ---------------------------------------------------------------- the row-kernel table
def _case(name, k, F, lengths):
    return RowCase(name, k, F, tuple(lengths), *row_kernel(k, F, max(lengths)))


ROW_CASES = [_case(*c) for c in [
    ("lds_small", 7, 5, (12, 0, 1, 2, 5, 11)),
    ("lds_big", 13, 8, (20, 0, 1, 3, 19)),  # above the 64 KiB a launch gets without the attribute
    ("lds_last", 13, 8, (36, 0, 1, 35)),  # the last row length whose four samples fit the LDS share ...
    ("coop_first", 13, 8, (37, 0, 1, 36)),  # ... and the first that gets the workgroup to itself
    ("coop_big_L32", 50, 8, (20, 0, 1, 2, 19)),
    ("coop_last_L64", 100, 4, (37, 0, 1, 36)),  # the last that fits at all ...
    ("generic_size_L64", 100, 4, (38, 0, 1, 37)),  # ... and the first that does not: R = 1 in the generic kernel
    ("lds_row64", 3, 3, (64, 0, 1, 63)),  # lane 63 holds an entry: 1ull << 63 in the field masks
    ("generic_row65", 3, 3, (65, 0, 1, 64, 63)),
    ("coop_F64_m64_L1", 1, 64, (64, 0, 1, 63)),  # both limits of 64 at once
    ("generic_F65", 1, 65, (9, 0, 1, 8)),  # nb > 64
    ("lds_big_k128", 128, 2, (10, 0, 1, 9)),  # no padding component: the widest row there is
    ("lds_L16", 30, 6, (16, 0, 1, 15)),
    # the rest of the cross product: every L under every kernel, two lane widths on either side of 64 KiB per LDS kernel
    ("lds_L1", 1, 3, (9, 0, 1, 2, 8)),
    ("lds_L32", 50, 3, (10, 0, 1, 9)),
    ("lds_L64", 100, 2, (7, 0, 1, 6)),
    ("coop_L2", 3, 40, (40, 0, 1, 2, 39)),
    ("coop_big_L4", 7, 30, (40, 0, 1, 39)),
    ("coop_L16", 30, 6, (30, 0, 1, 2, 29)),
    ("generic_L4", 7, 5, (66, 0, 1, 2, 65)),
    ("generic_L8", 13, 65, (9, 0, 1, 8)),
    ("generic_size_L16", 30, 10, (61, 0, 1, 60)),  # 156 256 B; 59 entries (152 064 B) would still fit
    ("generic_L32", 50, 3, (70, 0, 1, 64, 65)),
]]
ROW_BY_NAME = {c.name: c for c in ROW_CASES}
# (below, above): the two sides of each threshold of run_ffm
THRESHOLD_PAIRS = [("lds_last", "coop_first"), ("coop_last_L64", "generic_size_L64"), ("lds_row64", "generic_row65"),
                   ("coop_F64_m64_L1", "generic_F65")]
# one case per kernel for the four (fitLinear, fitIntercept) settings.  (Not lds_small: without the linear term AdaGrad's loss on
# it does not fall from the first epoch to the second in the oracle, 0.59649 -> 0.59662, and such a fit is not asked to compare.)
FLAG_CASES = ("lds_big", "coop_first", "generic_row65")
FLAGS = [(True, True), (True, False), (False, True), (False, False)]  # (fitLinear, fitIntercept)


@functools.lru_cache(maxsize=None)
def row_data(name):
    """(FieldCsr, y) of a row case: shared between callers and read-only"""
    c = ROW_BY_NAME[name]
    X = lengths_ffm(c.lengths, N_TRAIN, D_TRAIN, c.F, seed=[c.k, c.F, len(c.lengths), max(c.lengths)])
    return X, targets(N_TRAIN, N_TRAIN + c.k)


@functools.lru_cache(maxsize=None)
def row_perms(n=N_TRAIN):
    """the orders of the two epochs.  The first starts with row 0, the longest: AdaGrad's first mini-batch is that one sample."""
    rng = np.random.default_rng(7)
    perms = np.stack([rng.permutation(n) for _ in range(EPOCHS)]).astype(np.int64)
    at = int(np.flatnonzero(perms[0] == 0)[0])
    perms[0, [0, at]] = perms[0, [at, 0]]
    perms.setflags(write=False)
    return perms


def row_launches(solver, n=N_TRAIN, batch=BATCH):
    """row-phase launches of a fit: one per mini-batch"""
    return len(fit_batches(n, batch, solver))


# ---------------------------------------------------------------- the column path
COL_F, COL_D, COL_N, COL_BATCH = 3, 400, 450, 150
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 150)  # either side of kFtab and of kHeavyTouches; 129: segments of 64, 64 and 1
CONTROL_COUNTS = (1, 2, 63, 64, 65, 127, 128, 128, 128)  # nothing for the heavy path
COL_KS = (1, 13, 50, 100)
COL_CAPS = (1.0, 16.0)  # SGD's touch cap: at 16 a feature of 65 touches takes the pow branch of ffm_touch_factors with c = 65 / 16


@functools.lru_cache(maxsize=None)
def col_data(control=False):
    """COL_N rows in storage order; in every block of COL_BATCH rows feature c < 9 is in exactly counts[c] rows, the block's
    first among them (so the windows AdaGrad's first epoch moves by one row keep their counts, and the last one loses one per
    feature: 128 and 149 touches), and every row has three more features from the other ids.  Odd rows are stored unsorted."""
    counts = CONTROL_COUNTS if control else COUNTS
    rng = np.random.default_rng(150 + int(control))
    field_of = fields_of(COL_D, COL_F, rng)
    rows = [[] for _ in range(COL_N)]
    for lo in range(0, COL_N, COL_BATCH):
        for c, cnt in enumerate(counts):
            for r in [0] + (1 + rng.choice(COL_BATCH - 1, size=cnt - 1, replace=False)).tolist():
                rows[lo + r].append(c)
    idx, vals, indptr = [], [], [0]
    for i, r in enumerate(rows):
        row = np.sort(np.array(r + (len(counts) + rng.choice(COL_D - len(counts), size=3, replace=False)).tolist(), dtype=np.int64))
        if i % 2:
            row = rng.permutation(row)
            if np.all(np.diff(row) > 0):
                row = row[::-1]
        idx.append(row)
        vals.append(rng.uniform(-1, 1, size=len(row)))
        indptr.append(indptr[-1] + len(row))
    idx = np.concatenate(idx)
    return FieldCsr(indptr, idx, np.concatenate(vals), field_of[idx], COL_N, COL_D, COL_F), targets(COL_N, 151 + int(control))


# ---------------------------------------------------------------- the refresh
REFRESH = {"dense": 40, "sparse": 30000}  # regime -> d; batch COL_BATCH, COL_N rows, COL_F fields
REFRESH_KS = (1, 50, 100)
REFRESH_LENGTHS = (8, 0, 1, 2, 3, 5, 7)


@functools.lru_cache(maxsize=None)
def refresh_data(regime):
    """dense: a batch's touches are at least four times its unique features, k_ffm_refresh runs in front of every batch but
    AdaGrad's stored first one; sparse: nowhere.  Storage order."""
    d = REFRESH[regime]
    X = lengths_ffm(REFRESH_LENGTHS, COL_N, d, COL_F, seed=[d, COL_N])
    return X, targets(COL_N, d)


# ---------------------------------------------------------------- decisionFunction
PREDICT_KS = (1, 3, 7, 13, 30, 50, 100, 128)  # L = 1, 2, 4, 8, 16, 32, 64, 64
PREDICT_FS = (1, 3, 65)
PREDICT_LENGTHS = (130, 0, 1, 2, 63, 64, 65)
N_PREDICT, D_PREDICT = 261, 200
STRIDED_N = 40000  # above n_cu * 32 * 4 wavefronts (predict.hip:277-279) on 256 compute units: 32 768


@functools.lru_cache(maxsize=None)
def predict_data(F):
    """261 rows of 0 to 130 entries, the odd ones unsorted.  Every fifth row, where it has two entries or more, has its first column id
    once more at its end, with another value: INTEGRATION.md section 1 defines decisionFunction of such a row, and the j1 < j2
    test of k_ffm_predict (predict.hip:248) skips the pair of the two."""
    base = lengths_ffm(PREDICT_LENGTHS, N_PREDICT, D_PREDICT, F, seed=[F, N_PREDICT], hubs=N_HUBS)
    rng = np.random.default_rng(F)
    field_of = np.zeros(D_PREDICT, np.int64)
    field_of[base.indices] = base.fields
    idx, vals, indptr = [], [], [0]
    for i in range(base.n):
        row, x = base.row(i), base.data[base.indptr[i]:base.indptr[i + 1]]
        if i % 5 == 2 and len(row) >= 2:
            row, x = np.append(row, row[0]), np.append(x, rng.uniform(-1, 1))
        idx.append(row)
        vals.append(x)
        indptr.append(indptr[-1] + len(row))
    idx = np.concatenate(idx)
    return FieldCsr(indptr, idx, np.concatenate(vals), field_of[idx], base.n, D_PREDICT, F)


@functools.lru_cache(maxsize=None)
def strided_data(n=STRIDED_N, d=50, F=2):
    """rows of 0 to 3 entries, more samples than the grid of k_ffm_predict has wavefronts: its loop runs a second pass for some
    of them only"""
    rng = np.random.default_rng(n)
    field_of = fields_of(d, F, rng)
    lens = rng.integers(0, 4, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    three = np.argsort(rng.random((n, d)), axis=1)[:, :3]  # distinct ids per row, in no order
    idx = three[np.arange(3)[None, :] < lens[:, None]].astype(np.int64)
    return FieldCsr(indptr, idx, rng.uniform(-1, 1, size=len(idx)), field_of[idx], n, d, F)
