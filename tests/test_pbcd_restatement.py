"""CPU: the plain-Python restatement of proximal block coordinate descent (tests/pbcd_restatement.py) that the device tests
hold the library to.  (1) It agrees with a dense brute-force PBCD -- every derivative from the ANOVA kernel's definition
over the other features, every prox from the whole current P, the prediction recomputed from the model after every step --
on the reference's grid (tests/test_pbcd_{l1,l21,squaredl21}.nim) within the reference's own tolerance for that comparison
(checkAlmostEqual's defaults, tests/utils.nim:82-105: rtol 1e-6, atol 1e-9; 1e-7 on the intercept).  (2) CD's level
schedule gives the reference's bits for L1 and L21; the run schedule does for SquaredL21, and the level schedule does NOT:
its prox reads the running sum of every row's norm.  (3) The input of the device's re-sum case takes SquaredL21's re-sum
branch (squaredl21.nim:37-38)."""
import itertools

import numpy as np
import pytest

import pbcd_restatement as R
from common import init_fm, make_fm_dataset
from test_cd_restatement import _matrices, anova_slow, predict_slow
from test_pcd_restatement import _example_012

N, D, K = 50, 6, 4
REGS = ("l1", "l21", "squaredl21")
RESUM_SEED = 45  # tests/test_gpu_pbcd.py::test_resum_branch runs the same input on the device


def prox_slow(reg, Po, j, lam):
    """the prox of row j from the whole current P[order] ([k][d + nAug]), after P[:, j] -= grad / invStepSize"""
    pj = Po[:, j].copy()
    if reg == "l1":
        return np.array([R.softthreshold(v, lam) for v in pj])
    if reg == "l21":
        nrm = np.sqrt((pj ** 2).sum())
        return pj * (1.0 - lam / nrm) if nrm > lam else np.zeros_like(pj)
    pj /= 1 + 2 * lam
    nrm = np.sqrt((pj ** 2).sum())
    strength = sum(np.sqrt((Po[:, t] ** 2).sum()) for t in range(Po.shape[1]) if t != j)
    lam_scaled = 2.0 * lam / (1.0 + 2 * lam) * strength
    return pj * (1.0 - lam_scaled / nrm) if nrm > lam_scaled else np.zeros_like(pj)


def pbcd_slow(Xd, y, P, w, b, degree, n_aug, fit_linear, fit_intercept, maxIter, reg, alpha0=1e-6, alpha=1e-3, beta=1e-4,
              gamma=1e-4):
    """dense brute-force PBCD, squared loss: alpha0 and alpha times nSamples, beta and gamma as given (pbcd.nim:226-227)"""
    n, d = Xd.shape
    Xa = np.hstack([Xd, np.ones((n, n_aug))])
    P, w = P.copy(), w.copy()
    a0n, an = alpha0 * n, alpha * n
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
            for j in range(d + n_aug):
                others = [t for t in range(d + n_aug) if t != j]
                dA = np.array([[anova_slow(Xa[i, others], P[o, s, others], deg - 1) * Xa[i, j] for s in range(P.shape[1])]
                               for i in range(n)])
                grad = ((yp - y)[:, None] * dA).sum(0) / n + beta * P[o, :, j]
                inv = max((dA ** 2).sum() / n + beta, 1e-12)
                P[o, :, j] -= grad / inv
                P[o, :, j] = prox_slow(reg, P[o], j, gamma / inv)
                yp = predict_slow(Xa, P, w, b, degree)
    return P, w, b


def _grid():
    return [(reg, degree, fit_lower) for reg in REGS for degree in ((2,) if reg == "squaredl21" else (2, 3, 4))
            for fit_lower in ("explicit", "none", "augment")]


@pytest.mark.parametrize("reg,degree,fit_lower", _grid())
def test_restatement_matches_brute_force(reg, degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, Xd, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(D, degree, K, fit_lower, fit_linear, seed=1)
        P, w, b, _, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                              maxIter=3, tol=0.0, beta=1e-5, gamma=1e-5, reg=reg)
        Ps, ws, bs = pbcd_slow(Xd, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, 3, reg, beta=1e-5, gamma=1e-5)
        tag = (reg, degree, fit_lower, fit_linear, fit_intercept)
        assert abs(b - bs) < 1e-7, tag
        np.testing.assert_allclose(w, ws, rtol=1e-6, atol=1e-9, err_msg=str(tag))
        np.testing.assert_allclose(P, Ps, rtol=1e-6, atol=1e-9, err_msg=str(tag))


def _fit_orders(name, reg, degree, fit_lower, gamma, orders=("reference", "level", "run")):
    indptr, indices, data, n, d = _matrices()[name]
    y = np.random.default_rng(9).standard_normal(n)
    P0, w0, b0, n_aug = init_fm(d, degree, 3, fit_lower, True, seed=2, scale=0.1)
    args = (indptr, indices, data, y, P0, w0, 0.1, degree, n_aug, True, True)
    kw = dict(maxIter=3, tol=0.0, gamma=gamma, reg=reg)
    return {o: R.fit(*args, order=o, **kw) for o in orders}


def _same(a, b):
    """P, w, the intercept and viol bit for bit; the running loss total is summed in the order of the walk"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and \
        [v for v, _ in a[3]] == [v for v, _ in b[3]] and np.allclose([l for _, l in a[3]], [l for _, l in b[3]], rtol=1e-12)


@pytest.mark.parametrize("name", ["user_item", "ragged_unsorted", "random_sparse", "unsorted"])
@pytest.mark.parametrize("reg,degree,fit_lower", [("l1", 2, "explicit"), ("l1", 3, "augment"), ("l21", 2, "explicit"),
                                                  ("l21", 3, "explicit"), ("l21", 3, "augment")])
def test_level_order_is_bit_equal_for_l1_and_l21(name, reg, degree, fit_lower):
    fits = _fit_orders(name, reg, degree, fit_lower, 1e-3)
    assert _same(fits["reference"], fits["level"])
    assert _same(fits["reference"], fits["run"])


@pytest.mark.parametrize("name", ["user_item", "ragged_unsorted", "random_sparse", "unsorted"])
@pytest.mark.parametrize("fit_lower", ["explicit", "augment"])
def test_run_order_is_bit_equal_for_squaredl21(name, fit_lower):
    fits = _fit_orders(name, "squaredl21", 2, fit_lower, 1e-3, orders=("reference", "run"))
    assert _same(fits["reference"], fits["run"])


def _fit_example(reg, order):
    indptr, indices, data, n, d = _example_012()
    y = np.array([1.0, -0.5, 2.0])
    P0 = np.array([[[0.3, -0.2, 0.4], [0.1, 0.5, -0.3]]])
    return R.fit(indptr, indices, data, y, P0, np.zeros(d), 0.0, 2, 0, False, False, maxIter=2, tol=0.0, beta=1e-3, gamma=0.05,
                 reg=reg, order=order)


def test_level_order_differs_for_squaredl21():
    """the three-column example of DESIGN.md section 13: level order 0, 2, 1 against the chain's 0, 1, 2.  With L21 in
    SquaredL21's place the level order is the reference's again: the difference is the chain."""
    ref = _fit_example("squaredl21", "reference")
    assert _same(ref, _fit_example("squaredl21", "run"))
    assert not np.array_equal(ref[0], _fit_example("squaredl21", "level")[0])
    assert _same(_fit_example("l21", "reference"), _fit_example("l21", "level"))


def test_resum_branch_is_taken():
    """strong regularisation from the reference's alpha0 = alpha = beta = gamma = 1e5 grid: the rows collapse, the running
    cache falls below norms[j] by rounding and is summed again (squaredl21.nim:37-38)"""
    Xo, _, y = make_fm_dataset(N, D, 2, K, RESUM_SEED, "explicit", True, True, scale=1.0)
    P0, w0, b0, n_aug = init_fm(Xo.d, 2, K, "explicit", True, seed=1, scale=0.1)
    for order in ("reference", "run"):
        R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, 0.05, 2, n_aug, True, True, maxIter=5, tol=0.0, alpha0=1e5, alpha=1e5,
              beta=1e5, gamma=1e5, reg="squaredl21", order=order)
        assert R.last_resums > 0


def test_refusals():
    args = ([0, 1], [0], [1.0], [1.0], np.zeros((1, 2, 1)), np.zeros(1), 0.0)
    with pytest.raises(ValueError, match="PBCD cannot be used for squaredl12."):
        R.fit(*args, 2, 0, False, False, reg="squaredl12")
    with pytest.raises(ValueError, match="transpose=true is not supported for BCD."):
        R.fit(*args, 2, 0, False, False, reg="squaredl21", transpose=True)
    with pytest.raises(ValueError, match="SquaredL21 supports only degree=2."):
        R.fit(*args, 3, 0, False, False, reg="squaredl21")
