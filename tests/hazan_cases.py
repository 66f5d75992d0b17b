"""Fixed inputs of the Hazan tests (tests/test_hazan_restatement.py on the CPU, tests/test_gpu_hazan.py on the device), all
generated from seeds.

Conditioning decides what can be compared at all: the gradient matrix of a nearly fitted or very noisy residual has a tiny
eigengap, and the power method then amplifies rounding differences enormously.  The inputs therefore plant factors of
distinct scales, keep the label noise at 0.02 and the one long row small; tests/test_hazan_restatement.py guards every case
used on the device (tree sums against in-order sums below 1e-8 relative)."""
import itertools

import numpy as np

from hazan_restatement import Data

GRID = dict(n=50, d=6, maxComponents=6, maxIter=12, maxIterPower=200, tolPower=0.0, tol=-100.0, eta=3.0)
WIDE = dict(n=2500, d=300, maxComponents=3, maxIter=5, maxIterPower=100, tolPower=0.0, tol=-100.0, eta=4.0)
SCALES = np.array([1.0, 0.6, 0.35])  # the planted factors' weights: distinct, so the eigengap is wide


def grid_flags():
    """optimal x ignoreDiag x fitLinear x fitIntercept"""
    return list(itertools.product([True, False], repeat=4))


def _csr(Xd):
    n, d = Xd.shape
    mask = Xd != 0.0
    indptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1)))).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return Data(indptr, cols.astype(np.int64), Xd[rows, cols], n, d)


def _anova2(Xd, p):
    a = Xd @ p
    return 0.5 * (a * a - (Xd * Xd) @ (p * p))


def _targets(Xd, rng, fitLinear, fitIntercept, sign=1.0, scales=SCALES):
    n, d = Xd.shape
    y = np.zeros(n)
    for s, lam in enumerate(scales):
        p = rng.normal(size=d)
        y += sign * lam * _anova2(Xd, p / np.linalg.norm(p)) * d
    if fitLinear:
        y += Xd @ rng.normal(scale=0.5, size=d)
    if fitIntercept:
        y += 0.7
    return y + rng.normal(scale=0.02, size=n)


def grid_data(fitLinear, fitIntercept, sign=1.0, scales=SCALES):
    """n = 50, d = 6, about 70 % of the entries stored"""
    rng = np.random.default_rng(42)
    Xd = rng.uniform(-1.0, 1.0, size=(GRID["n"], GRID["d"])) * (rng.uniform(size=(GRID["n"], GRID["d"])) > 0.3)
    return _csr(Xd), _targets(Xd, rng, fitLinear, fitIntercept, sign, scales)


# the power-stop test: one planted factor far above the others, so that |eval - evalOld| falls by more than 4x per iteration
# and the stop has a margin on both sides
POWER_STOP_SCALES = np.array([1.0, 0.03, 0.01])
POWER_STOP_FLAGS = [(True, True, True, True), (True, False, False, True), (False, True, True, False), (False, False, False, False)]


def wide_data():
    """n = 2500, d = 300, about 8 entries per row; column 0 holds every non-empty row, row 7 holds 200 small entries, row 11
    and column 299 are empty"""
    n, d = WIDE["n"], WIDE["d"]
    rng = np.random.default_rng(7)
    Xd = np.zeros((n, d))
    for i in range(n):
        cols = rng.choice(np.arange(1, d - 1), size=7, replace=False)
        Xd[i, cols] = rng.uniform(-1.0, 1.0, size=7)
    Xd[:, 0] = rng.uniform(0.2, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    Xd[7, :] = 0.0
    Xd[7, rng.choice(np.arange(0, d - 1), size=200, replace=False)] = rng.uniform(-0.15, 0.15, size=200)
    Xd[7, 0] = 0.1
    Xd[11, :] = 0.0
    Xd[:, d - 1] = 0.0
    y = np.zeros(n)
    for s, lam in enumerate(SCALES):
        p = np.zeros(d)
        sup = rng.choice(np.arange(0, d - 1), size=40, replace=False)
        p[sup] = rng.normal(size=40)
        p[0] = 1.0
        y += lam * _anova2(Xd, p / np.linalg.norm(p)) * 8.0
    y += Xd @ rng.normal(scale=0.3, size=d) + 0.5
    return _csr(Xd), y + rng.normal(scale=0.02, size=n)


# (ignoreDiag, optimal, fitLinear, fitIntercept) of the wide case: both kernels and both step rules with the linear part, once
# with neither the linear term nor the intercept
WIDE_RUNS = [(True, True, True, True), (True, False, True, True), (False, True, True, True), (False, False, True, True),
             (True, True, False, False)]


def numpy_starts(seed):
    """callable(outer, d) -> the power method's start vector, U(-1, 1)"""
    return lambda outer, d: np.random.default_rng(seed + outer).uniform(-1.0, 1.0, size=d)


def nim_starts(seed, count, d):
    """the start vectors the host draws after randomize(seed): 2 * rand(1.0) - 1.0, d draws per outer iteration from the one
    global stream (tensor/tensor.nim:920-921); the generator is the library's host-side restatement (no device needed)"""
    import nimfm_amd as nf

    rng = nf.NimRand(seed)
    vs = [2 * rng.rand(d, 1.0) - 1.0 for _ in range(count)]
    return lambda outer, d_: vs[outer]
