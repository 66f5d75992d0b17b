"""CPU: the plain-Python restatement of coordinate descent (tests/cd_restatement.py) that the device tests hold the library
to.  (1) It agrees with a brute-force CD after tests/optimizer/cd_slow.nim -- every derivative by enumerating the
combinations of the other features, the prediction recomputed from scratch after every step -- on the reference's grid
(test_cd.nim:92-127).  (2) Walking the features of every level in the level schedule, reversed inside each level, gives
the same bits as the reference's ascending loop: the claim the device kernels rest on."""
import itertools

import numpy as np
import pytest

import cd_restatement as R
from common import init_fm, make_fm_dataset, random_csr

N, D, K = 50, 6, 4


def anova_slow(x, p, deg):
    """the ANOVA kernel of degree deg by enumerating the combinations (kernels_slow.nim)"""
    total = 0.0
    for idx in itertools.combinations(range(len(x)), deg):
        prod = 1.0
        for j in idx:
            prod *= p[j] * x[j]
        total += prod
    return total


def predict_slow(Xa, P, w, b, degree):
    d = len(w)
    out = np.full(Xa.shape[0], b)
    out += Xa[:, :d] @ w
    for o in range(P.shape[0]):
        for s in range(P.shape[1]):
            out += np.array([anova_slow(Xa[i], P[o, s], degree - o) for i in range(Xa.shape[0])])
    return out


def cd_slow(Xd, y, P, w, b, degree, n_aug, fit_linear, fit_intercept, maxIter, alpha0=1e-6, alpha=1e-3, beta=1e-3):
    """tests/optimizer/cd_slow.nim + fit_linear_slow.nim, squared loss"""
    n, d = Xd.shape
    Xa = np.hstack([Xd, np.ones((n, n_aug))])
    P, w = P.copy(), w.copy()
    a0n, an, bn = alpha0 * n, alpha * n, beta * n
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
                    dA = np.zeros(n)
                    for i in range(n):
                        others = [t for t in range(d + n_aug) if t != j]
                        dA[i] = anova_slow(Xa[i, others], P[o, s, others], deg - 1) * Xa[i, j]
                    inv = (dA ** 2).sum() + bn
                    u = (bn * P[o, s, j] + ((yp - y) * dA).sum()) / inv
                    P[o, s, j] -= u
                    yp = predict_slow(Xa, P, w, b, degree)
    return P, w, b


@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_restatement_matches_brute_force(degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, Xd, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(D, degree, K, fit_lower, fit_linear, seed=1)
        P, w, b, _, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                              maxIter=3, tol=0.0)
        Ps, ws, bs = cd_slow(Xd, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, maxIter=3)
        tag = (degree, fit_lower, fit_linear, fit_intercept)
        assert abs(b - bs) < 1e-7, tag
        np.testing.assert_allclose(w, ws, rtol=1e-6, atol=1e-8, err_msg=str(tag))
        np.testing.assert_allclose(P, Ps, rtol=1e-6, atol=1e-8, err_msg=str(tag))


def _user_item(n_users, n_items, n, seed):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n_users, n), rng.integers(0, n_items, n)], 1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    m = len(pairs)
    return np.arange(0, 2 * m + 1, 2), np.stack([pairs[:, 0], n_users + pairs[:, 1]], 1).reshape(-1), np.ones(2 * m), m, n_users + n_items


def _ragged(n, d, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.choice(d, rng.integers(0, min(d, 30) + 1), replace=False) for _ in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return indptr, np.concatenate(rows), rng.uniform(-1, 1, indptr[-1]), n, d


def _matrices():
    out = {"user_item": _user_item(20, 30, 150, 1), "ragged_unsorted": _ragged(60, 40, 2)}
    Xo = random_csr(80, 30, 8, seed=3, sorted_idx=True)
    out["random_sparse"] = (Xo.indptr, Xo.indices, Xo.data, Xo.n, Xo.d)
    Xu = random_csr(70, 25, 6, seed=4, sorted_idx=False)
    out["unsorted"] = (Xu.indptr, Xu.indices, Xu.data, Xu.n, Xu.d)
    return out


@pytest.mark.parametrize("name", ["user_item", "ragged_unsorted", "random_sparse", "unsorted"])
@pytest.mark.parametrize("degree,fit_lower", [(2, "explicit"), (3, "explicit"), (3, "augment")])
def test_level_order_is_bit_equal(name, degree, fit_lower):
    indptr, indices, data, n, d = _matrices()[name]
    y = np.random.default_rng(9).standard_normal(n)
    P0, w0, b0, n_aug = init_fm(d, degree, 3, fit_lower, True, seed=2, scale=0.1)
    args = (indptr, indices, data, y, P0, w0, 0.1, degree, n_aug, True, True)
    seq = R.fit(*args, maxIter=3, tol=0.0)
    lvl = R.fit(*args, maxIter=3, tol=0.0, level_order=True)
    assert np.array_equal(seq[0], lvl[0]) and np.array_equal(seq[1], lvl[1]) and seq[2] == lvl[2]
    assert seq[3] == lvl[3]


def test_user_item_schedule_depth():
    indptr, indices, _, n, d = _user_item(20, 30, 150, 1)
    depth, widest = R.schedule_depth(indptr, indices, n, d)
    assert depth == 2
