"""CPU: the plain-Python restatement of proximal coordinate descent (tests/pcd_restatement.py) that the device tests hold
the library to.  (1) It agrees with a brute-force PCD after tests/optimizer/pcd_slow.nim -- every derivative by
enumerating the combinations of the other features, every prox from the whole current P (regularizer/*_slow.nim), the
prediction recomputed after every step -- on the reference's grid.  (2) The run schedule gives the reference's bits for
every regulariser; CD's level schedule does for L1 and row-wise SquaredL12, and does NOT for column-wise SquaredL12,
whose prox reads a running sum over every earlier feature: the reason the library has a second schedule."""
import itertools

import numpy as np
import pytest

import pcd_restatement as R
from common import init_fm, make_fm_dataset, random_csr
from test_cd_restatement import _matrices, _user_item, anova_slow, predict_slow

N, D, K = 50, 6, 4
REGS = [("l1", False), ("squaredl12", False), ("squaredl12", True), ("omegati", False)]


def prox_slow(reg, transpose, Po, s, j, lam, deg):
    """regularizer/*_slow.nim prox(P, lam, degree, s, j) on P[order] ([k][d + nAug]), after P[s, j] -= update"""
    psj = Po[s, j]
    if reg == "l1":
        return R.softthreshold(psj, lam)
    if reg == "squaredl12":
        strength = np.abs(Po[s]).sum() if transpose else np.abs(Po[:, j]).sum()
        strength -= abs(psj)
        return R.softthreshold(psj / (1 + 2 * lam), 2 * lam * strength / (1 + 2 * lam))
    absp = np.abs(Po[s]).copy()
    absp[j] = 0.0
    return R.softthreshold(psj, lam * anova_slow(np.ones(len(absp)), absp, deg - 1))


def pcd_slow(Xd, y, P, w, b, degree, n_aug, fit_linear, fit_intercept, maxIter, reg, transpose, alpha0=1e-6, alpha=1e-3,
             beta=1e-4, gamma=1e-4):
    """tests/optimizer/pcd_slow.nim + fit_linear_slow.nim, squared loss"""
    n, d = Xd.shape
    Xa = np.hstack([Xd, np.ones((n, n_aug))])
    P, w = P.copy(), w.copy()
    a0n, an, bn, gn = alpha0 * n, alpha * n, beta * n, gamma * n
    colsq = (Xd ** 2).sum(0)
    yp = predict_slow(Xa, P, w, b, degree)
    for _ in range(maxIter):
        if fit_intercept:
            r = (a0n * b + (yp - y).sum()) / (n + a0n)
            b -= r
            yp = predict_slow(Xa, P, w, b, degree)
        if fit_linear:
            for j in range(d):
                u = (an * w[j] + ((yp - y) * Xd[:, j]).sum()) / (colsq[j] + an)
                w[j] -= u
                yp -= u * Xd[:, j]
            yp = predict_slow(Xa, P, w, b, degree)
        for o in range(P.shape[0]):
            deg = degree - o
            for s in range(P.shape[1]):
                for j in range(d + n_aug):
                    others = [t for t in range(d + n_aug) if t != j]
                    dA = np.array([anova_slow(Xa[i, others], P[o, s, others], deg - 1) * Xa[i, j] for i in range(n)])
                    inv = (dA ** 2).sum() + bn
                    if inv < 1e-12:
                        continue
                    u = (bn * P[o, s, j] + ((yp - y) * dA).sum()) / inv
                    P[o, s, j] -= u
                    P[o, s, j] = prox_slow(reg, transpose, P[o], s, j, gn / inv, deg)
                    yp = predict_slow(Xa, P, w, b, degree)
    return P, w, b


def _grid():
    out = []
    for reg, tr in REGS:
        degrees = (2,) if reg == "squaredl12" else (2, 3, 4)
        for degree, fit_lower in itertools.product(degrees, ("explicit", "none", "augment")):
            out.append((reg, tr, degree, fit_lower))
    return out


@pytest.mark.parametrize("reg,transpose,degree,fit_lower", _grid())
def test_restatement_matches_brute_force(reg, transpose, degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, Xd, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(D, degree, K, fit_lower, fit_linear, seed=1)
        P, w, b, _, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                              maxIter=3, tol=0.0, gamma=1e-3, reg=reg, transpose=transpose)
        Ps, ws, bs = pcd_slow(Xd, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, 3, reg, transpose, gamma=1e-3)
        tag = (reg, transpose, degree, fit_lower, fit_linear, fit_intercept)
        assert abs(b - bs) < 1e-7, tag
        np.testing.assert_allclose(w, ws, rtol=1e-7, atol=1e-9, err_msg=str(tag))
        np.testing.assert_allclose(P, Ps, rtol=1e-7, atol=1e-9, err_msg=str(tag))


def _fit_orders(name, reg, transpose, degree, fit_lower, gamma):
    indptr, indices, data, n, d = _matrices()[name]
    y = np.random.default_rng(9).standard_normal(n)
    P0, w0, b0, n_aug = init_fm(d, degree, 3, fit_lower, True, seed=2, scale=0.1)
    args = (indptr, indices, data, y, P0, w0, 0.1, degree, n_aug, True, True)
    kw = dict(maxIter=3, tol=0.0, gamma=gamma, reg=reg, transpose=transpose)
    return {o: R.fit(*args, order=o, **kw) for o in ("reference", "level", "run")}


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("name", ["user_item", "ragged_unsorted", "random_sparse", "unsorted"])
@pytest.mark.parametrize("reg,degree,fit_lower", [("squaredl12", 2, "explicit"), ("squaredl12", 2, "augment"),
                                                  ("omegati", 2, "explicit"), ("omegati", 3, "explicit"),
                                                  ("omegati", 3, "augment")])
def test_run_order_is_bit_equal_for_chained(name, reg, degree, fit_lower):
    fits = _fit_orders(name, reg, True, degree, fit_lower, 1e-3)
    assert _same(fits["reference"], fits["run"])


@pytest.mark.parametrize("name", ["user_item", "ragged_unsorted", "random_sparse", "unsorted"])
@pytest.mark.parametrize("reg,transpose,degree,fit_lower", [("l1", False, 2, "explicit"), ("l1", False, 3, "augment"),
                                                            ("squaredl12", False, 2, "explicit"),
                                                            ("squaredl12", False, 2, "augment")])
def test_level_order_is_bit_equal_for_local(name, reg, transpose, degree, fit_lower):
    fits = _fit_orders(name, reg, transpose, degree, fit_lower, 1e-3)
    assert _same(fits["reference"], fits["level"])
    assert _same(fits["reference"], fits["run"])


def _example_012():
    """columns 0 and 1 share sample 0, column 2 shares none: levels 1, 2, 1 -> level order 0, 2, 1; runs [0], [1, 2]"""
    indptr = np.array([0, 2, 3, 4])
    indices = np.array([0, 1, 1, 2])
    data = np.array([1.0, 0.5, -0.7, 1.3])
    return indptr, indices, data, 3, 3


def test_level_order_differs_for_columnwise_squaredl12():
    indptr, indices, data, n, d = _example_012()
    assert R.schedule(indptr, indices, n, d, False) == (2, 2)
    assert R.schedule(indptr, indices, n, d, True) == (2, 2)
    y = np.array([1.0, -0.5, 2.0])
    P0 = np.array([[[0.3, -0.2, 0.4], [0.1, 0.5, -0.3]]])
    kw = dict(maxIter=2, tol=0.0, beta=1e-3, gamma=0.05, reg="squaredl12", transpose=True)
    args = (indptr, indices, data, y, P0, np.zeros(d), 0.0, 2, 0, False, False)
    ref = R.fit(*args, order="reference", **kw)
    assert _same(ref, R.fit(*args, order="run", **kw))
    lvl = R.fit(*args, order="level", **kw)
    assert not np.array_equal(ref[0], lvl[0])
    assert (ref[0] == 0.0).any()  # the thresholds bite


def test_schedules_of_user_item():
    indptr, indices, _, n, d = _user_item(20, 30, 150, 1)
    assert R.schedule(indptr, indices, n, d, False)[0] == 2
    assert R.schedule(indptr, indices, n, d, True) == (2, 30)  # the users, then the items
    Xo = random_csr(80, 30, 8, seed=3, sorted_idx=True)
    runs = R.runs(R.columns(Xo.indptr, Xo.indices, Xo.data, Xo.n, Xo.d))
    assert [j for r in runs for j in r] == list(range(Xo.d))
