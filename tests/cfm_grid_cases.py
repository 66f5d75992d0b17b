"""Fixed inputs of the grid-edge tests of the convex factorization machine's two solvers (tests/test_cfm_grid_cases.py on the
CPU, tests/test_gpu_cfm_grid.py on the device), all generated from seeds and built sparse: hazan_restatement.Data straight
from indptr / indices / data, never a dense matrix (`broad` would need 5 GB).

The recipe is hazan_cases.wide_data's, because conditioning decides what can be compared: column 0 holds
every non-empty row with |value| in [0.2, 1], the other entries are U(-1, 1), the targets are three planted ANOVA factors with
hazan_cases.SCALES (each supported on 40 of the used columns plus column 0) plus a planted linear part on the used columns
plus 0.5, with label noise 0.02.  The row lengths cycle through CYCLE; one row holds small entries in 200 of the used columns
(in every used column where there are fewer), as wide_data's row 7 does.

    input      n        d        used columns                 what it is for
    tall       32 801   40       all but the last             more than 1024 workgroups of rows (n = 32 * 1025 + 1)
    long       262 401  40       all but the last             more than 1024 element-wise workgroups over n (256 * 1025 + 1)
    broad      2500     262 401  0..39, 32 768..32 799,       the partials of the column pass and of the element-wise passes
                                 262 144..262 175             over d and d + 1 from number 1024 on hold real mass
    edges_n    31..257  33       all                          the last workgroup of the row and element-wise passes over n
    edges_d    400/2500 31..256  all                          the dummy column as the last slot of a workgroup / alone in one
    cg_long    900      300      all but the last, 8 a row    a CG of more than kHazanChunk iterations in outer iteration 0
    cg_cap     10 000   30 000   all but the last, 8 a row    a CG that ends on its cap of kCgMaxIter iterations
    reuse      257      40     all but the last             the small fit after tall's on one solver and one model

tests/test_cfm_grid_cases.py asserts every one of these claims from the constants in the sources, and guards the conditioning
of every case the device file uses."""
import functools

import numpy as np

import gcd_cases as gc
import hazan_cases as hc
from hazan_restatement import Data

CYCLE = (0, 1, 7, 8, 9, 15, 16, 17, 3)  # every remainder of kG = 8 that ordered_acc's last round can meet, and the empty row
LONG_CYCLE = (1, 2, 3, 0)              # `long`: about 400 000 entries
LONG_ROW = 7                           # the row of small entries
BROAD_BANDS = ((0, 40), (32768, 32800), (262144, 262176))
EDGES_N = (31, 32, 33, 255, 256, 257)
EDGES_D = (31, 32, 255, 256)
EDGES_D_ROWS = {31: 400, 32: 400, 255: 2500, 256: 2500}  # 400 rows leave 256 columns ill-conditioned (a CG of 130 iterations)

# n, d, the used columns, the row-length cycle, the long row's index (None: none), the seed
SHAPES = {
    "tall": (32801, 40, np.arange(39), CYCLE, LONG_ROW, 11),
    "long": (262401, 40, np.arange(39), LONG_CYCLE, LONG_ROW, 12),
    "broad": (2500, 262401, np.concatenate([np.arange(a, b) for a, b in BROAD_BANDS]), CYCLE, LONG_ROW, 13),
    "cg_long": (900, 300, np.arange(299), (8,), None, 17),
    "cg_cap": (10000, 30000, np.arange(29999), (8,), None, 21),  # three times as many columns as rows: the CG ends on its cap
    "predict33": (33, 40, np.arange(39), CYCLE, LONG_ROW, 15),  # decisionFunction on rows that are not the training set
    "reuse": (257, 40, np.arange(39), CYCLE, LONG_ROW, 16),     # tall's width: the small fit that follows tall's on one model
}
for _n in EDGES_N:
    SHAPES["edges_n%d" % _n] = (_n, 33, np.arange(33), CYCLE, LONG_ROW, 100 + _n)
for _d in EDGES_D:
    SHAPES["edges_d%d" % _d] = (EDGES_D_ROWS[_d], _d, np.arange(_d), CYCLE, LONG_ROW, 400 + _d)

# Hazan's settings per input (hazan_cases.WIDE's, shortened: few outer iterations keep the late components' small eigengaps out)
HAZAN = {name: dict(maxComponents=3, maxIter=3, maxIterPower=40, tolPower=0.0, tol=-100.0, eta=4.0) for name in SHAPES}
HAZAN["long"].update(maxIter=2, maxIterPower=8)
HAZAN["cg_long"].update(maxIter=1)
HAZAN["cg_cap"].update(maxIter=1, maxIterPower=8)

# (ignoreDiag, optimal, fitLinear, fitIntercept) per input
_TT, _FF, _BARE = (True, True, True, True), (False, False, True, True), (True, True, False, False)
HAZAN_RUNS = [("tall", _TT), ("tall", _FF), ("tall", _BARE), ("broad", _TT), ("broad", _FF), ("broad", _BARE),
              ("long", _TT), ("long", (True, True, False, True))]
_EDGE_FLAGS = [(True, True, True, True), (False, True, True, True), (True, False, True, True), (False, False, True, True)]
# n = 31, 32, 33 with d = 33: Z^T Z has more columns than rows, the CG runs to the rank and rounding decides its result (tree
# against in-order sums: 1.7 relative on P), so these three fit the intercept alone (k_icpt); 255, 256 and 257 leave the same
# remainders of the 32 rows of a workgroup and run the CG
_NO_LINEAR = (True, True, False, True)
HAZAN_RUNS += [("edges_n%d" % n, _NO_LINEAR if n < 34 else _EDGE_FLAGS[k % 4]) for k, n in enumerate(EDGES_N)]
HAZAN_RUNS += [("edges_d%d" % d, _EDGE_FLAGS[(k + 1) % 4]) for k, d in enumerate(EDGES_D)]
CG_LONG_RUN = ("cg_long", (True, True, True, True))
CG_CAP_RUN = ("cg_cap", (True, True, True, True))  # no parity here (a CG that long is chaotic under rounding): counts and bits only
START_SEED = 100  # hazan_cases.numpy_starts(START_SEED): the power method's start vectors of every Hazan run here

# the power method at the edges of a chunk, on the reference grid
POWER_EDGES = (1, 31, 32, 33, 64, 65)
POWER_EDGE_FLAGS = (True, True, True, True)

# GreedyCD: gcd_cases.WIDE's settings with a shorter power method; nRefitting = 2 <= maxIterInner, so refitDiag runs
GCD = dict(gc.WIDE, maxIterPower=40)
GCD_CASES = ["tall:11", "tall:01", "long:11", "broad:11", "tall:11:logistic"]
GCD_POWER_EDGE = 33  # the chunk-edge count that also runs through GreedyCD, on its reference grid
GCD_GRID_CASE = "grid:11"


def _sparse(n, d, used, cycle, long_row, rng):
    """-> indptr, indices, data: row i holds cycle[i % len(cycle)] entries -- column 0 and distinct others of `used`, ascending"""
    used = np.asarray(used, dtype=np.int64)
    assert used[0] == 0 and (np.diff(used) > 0).all() and used[-1] < d
    m = len(used) - 1
    lens = np.array(cycle, dtype=np.int64)[np.arange(n) % len(cycle)]
    assert lens.max() - 1 <= m
    if n * m > 50_000_000:  # too large for the n x m draws below: row by row (no long row)
        assert long_row is None
        cols = [np.concatenate(([0], 1 + np.sort(rng.choice(m, size=L - 1, replace=False)))) if L else np.zeros(0, dtype=np.int64) for L in lens]
        vals = rng.uniform(-1.0, 1.0, size=int(lens.sum()))
        indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        first = indptr[:-1][lens > 0]
        vals[first] = rng.uniform(0.2, 1.0, size=len(first)) * rng.choice([-1.0, 1.0], size=len(first))
        return indptr, used[np.concatenate(cols).astype(np.int64)], vals
    ranks = np.argsort(np.argsort(rng.random((n, m)), axis=1), axis=1)  # a random order of the other columns per row
    mask = np.concatenate([(lens > 0)[:, None], ranks < (lens - 1)[:, None]], axis=1)
    vals = rng.uniform(-1.0, 1.0, size=(n, m + 1))
    vals[:, 0] = rng.uniform(0.2, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    if long_row is not None and long_row < n:
        k = min(200, m + 1)
        mask[long_row] = False
        mask[long_row, rng.choice(m + 1, size=k, replace=False)] = True
        mask[long_row, 0] = True
        vals[long_row] = rng.uniform(-0.15, 0.15, size=m + 1)
        vals[long_row, 0] = 0.1
    rows, pos = np.nonzero(mask)
    indptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1)))).astype(np.int64)
    return indptr, used[pos], vals[rows, pos]


def _row_sums(indptr, t, n):
    return np.bincount(np.repeat(np.arange(n), np.diff(indptr)), weights=t, minlength=n)


def _targets(indptr, indices, data, n, d, used, rng):
    """three planted ANOVA factors on 40 of the used columns plus column 0, a linear part on the used columns, 0.5, noise 0.02"""
    y = np.zeros(n)
    k = min(40, len(used) - 1)
    for lam in hc.SCALES:
        p = np.zeros(d)
        p[rng.choice(used[1:], size=k, replace=False)] = rng.normal(size=k)
        p[0] = 1.0
        p /= np.linalg.norm(p)
        t = data * p[indices]
        a = _row_sums(indptr, t, n)
        y += lam * 0.5 * (a * a - _row_sums(indptr, t * t, n)) * 8.0
    w = np.zeros(d)
    w[used] = rng.normal(scale=0.3, size=len(used))
    y += _row_sums(indptr, data * w[indices], n) + 0.5
    return y + rng.normal(scale=0.02, size=n)


@functools.lru_cache(maxsize=None)
def data(name):
    """-> (Data, y) of one input; computed once and shared, never modified"""
    n, d, used, cycle, long_row, seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    indptr, indices, vals = _sparse(n, d, used, cycle, long_row, rng)
    y = _targets(indptr, indices, vals, n, d, np.asarray(used, dtype=np.int64), rng)
    y.setflags(write=False)
    return Data(indptr, indices, vals, n, d), y


def hazan_kw(name, flags, **over):
    ignoreDiag, optimal, fitLinear, fitIntercept = flags
    return dict(HAZAN[name], ignoreDiag=ignoreDiag, optimal=optimal, fitLinear=fitLinear, fitIntercept=fitIntercept, **over)


def hazan_case(name, flags, **over):
    """-> (Data, y, keyword arguments of hazan_fit, start vectors); `grid` is the reference grid of hazan_cases"""
    if name == "grid":
        X, y = hc.grid_data(flags[2], flags[3])
        kw = dict(maxComponents=hc.GRID["maxComponents"], eta=hc.GRID["eta"], tol=hc.GRID["tol"], tolPower=0.0, ignoreDiag=flags[0],
                  optimal=flags[1], fitLinear=flags[2], fitIntercept=flags[3], maxIter=2, maxIterPower=hc.GRID["maxIterPower"])
        kw.update(over)
    else:
        X, y = data(name)
        kw = hazan_kw(name, flags, **over)
    return X, y, kw, hc.numpy_starts(START_SEED)


@functools.lru_cache(maxsize=None)
def hazan_plain(name, flags, maxIterPower=None):
    """the in-order restatement of one Hazan run with its stops live, computed once and shared (never modified)"""
    import hazan_restatement as hr
    X, y, kw, starts = hazan_case(name, flags, **({} if maxIterPower is None else dict(maxIterPower=maxIterPower)))
    return hr.hazan_fit(X, y, starts, **kw)


def gcd_case(name):
    """<input>:<ignoreDiag><fitLinear>[:<loss>] -> (Data, y, keyword arguments of gcd_fit), as gcd_cases.case"""
    shape, flags, lossname = (name.split(":") + [""])[:3]
    ig, fl = (c == "1" for c in flags)
    if shape == "grid":  # GreedyCD's reference grid, two outer iterations, the power method ending one past a chunk
        X, y = hc.grid_data(fl, True)
        return X, y, dict(gc.GRID, maxIter=2, maxIterInner=4, nRefitting=2, maxIterPower=GCD_POWER_EDGE, ignoreDiag=ig, fitLinear=fl,
                          fitIntercept=True)
    X, y = data(shape)
    kw = dict(GCD, ignoreDiag=ig, fitLinear=fl, fitIntercept=True)
    if lossname:
        return X, np.where(y > np.median(y), 1.0, -1.0), dict(kw, loss=lossname, task="classification")
    return X, y, kw


def predict_models(d, used):
    """the models of the decisionFunction cases: 0, 1 and 3 components on the used columns -> [(P, lams, w, intercept)]"""
    rng = np.random.default_rng(5)
    w = np.zeros(d)
    w[used] = rng.normal(size=len(used))
    P = np.zeros((3, d))
    P[:, used] = rng.normal(size=(3, len(used)))
    lams = np.array([0.5, -1.5, 2.0])
    return [(P[:k].copy(), lams[:k].copy(), w, 0.25) for k in (0, 1, 3)]
