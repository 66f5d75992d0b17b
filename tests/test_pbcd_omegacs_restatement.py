"""CPU: the plain-Python restatement of PBCD with OmegaCS (tests/pbcd_omegacs_restatement.py) that tests/test_gpu_pbcd_omegacs.py
holds the device to.  (a) It agrees with the brute-force prox of tests/regularizer/omegacs_slow.nim:28-45 -- every threshold lam
times the degree-(deg - 1) ANOVA polynomial of all current norms but row j's, nothing cached -- on the grid of
tests/test_pbcd_omegacs.nim:95-133, within the project's bound for restatement against brute force (rtol
1e-6, atol 1e-9, 1e-7 on the intercept; the reference's own bound here is atol 1e-5).  (b) The run schedule gives the
reference's bits, the level schedule does not: the prox reads the running polynomial of every row's norm.  (c) Both
exact-recompute branches (omegacs.nim:71-79 in prox, :60-61 in updateCacheBCD) are taken on the inputs the device test
runs.  (d) Every gamma the device file uses zeroes between 5 % and 95 % of the rows of P on the restatement, so no device
comparison passes on a prox that never (or always) thresholds.  (e) What the restatement refuses."""
import functools
import itertools

import numpy as np
import pytest

import cd_schedule_cases as S
import pbcd_omegacs_restatement as R
from common import init_fm, make_fm_dataset
from test_gpu_cd import user_item
from test_pcd_restatement import _example_012

N, D, K = 50, 6, 4
RECOMPUTE_SEEDS = {2: 45, 3: 42}  # degree -> make_fm_dataset's seed; tests/test_gpu_pbcd_omegacs.py runs the same inputs


@functools.lru_cache(maxsize=None)
def data_of(case):
    """(Xo, y) of a named input, shared and left unchanged"""
    if case in S.CASES:
        return S.inputs(case)
    return {"ui_60_80": lambda: user_item(60, 80, 900, seed=5), "ui_40_50": lambda: user_item(40, 50, 400, seed=7),
            "ui_30_40": lambda: user_item(30, 40, 300, seed=3), "ml100k": lambda: user_item(943, 1682, 100000, seed=11)}[case]()


# (case, degree, k, fitLower) -> gamma, sized by test_gamma_zeroes_some_rows_and_not_all below.  The share of zero rows is
# not monotone in gamma on ill-conditioned inputs: a value is moved only with that test's band in view, never the band.
GAMMA = {
    ("edges", 2, 4, "explicit"): 1e-5, ("edges", 3, 4, "explicit"): 1e-7,
    ("edges", 2, 3, "explicit"): 1e-5, ("edges", 2, 5, "explicit"): 1e-5, ("edges", 2, 32, "explicit"): 3e-5,
    ("edges", 2, 33, "explicit"): 3e-5, ("edges", 2, 64, "explicit"): 1e-4, ("edges", 2, 65, "explicit"): 1e-4,
    ("edges", 3, 3, "explicit"): 1e-7, ("edges", 3, 33, "explicit"): 1e-7,
    ("edges_gaps", 2, 4, "explicit"): 1e-5,  # at beta = alpha = 0
    ("long_1025", 2, 5, "explicit"): 3e-7, ("long_1025", 3, 5, "augment"): 1e-8, ("long_1025", 2, 65, "explicit"): 3e-6,
    ("ui_60_80", 2, 4, "explicit"): 1e-4, ("ui_60_80", 3, 4, "explicit"): 1e-4, ("ui_60_80", 3, 4, "augment"): 1e-6,
    ("ui_40_50", 2, 1, "explicit"): 1e-4, ("ui_40_50", 2, 130, "explicit"): 1e-4,
    ("ml100k", 2, 4, "explicit"): 1e-6,
}
# what a fit of the device file passes beside gamma, per case (tests/test_gpu_pbcd_omegacs.py reads it too)
FIT_KW = {"edges_gaps": dict(beta=0.0, alpha=0.0), "ml100k": dict(alpha0=1e-7, alpha=1e-5, beta=1e-3)}
ITERS = {"edges": 3, "edges_gaps": 3, "long_1025": 2, "ui_60_80": 3, "ui_40_50": 2, "ml100k": 2}


def restated(Xo, y, degree, fit_lower, fit_linear, fit_intercept, k=K, seed=1, **kw):
    """the restatement from S.start's values (tests/test_gpu_pbcd_omegacs.py::check_parity starts the device from the same)"""
    P0, w0, b0, n_aug = S.start(Xo, degree, k, fit_lower, fit_linear, fit_intercept, seed=seed)
    return R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, **kw)


# ---------------------------------------------------------------- (a) against brute force
@pytest.mark.parametrize("gamma", [1e-5, 3e-2])
@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_restatement_matches_brute_force(degree, fit_lower, gamma):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(D, degree, K, fit_lower, fit_linear, seed=1)
        args = (Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept)
        kw = dict(maxIter=3, tol=0.0, beta=1e-5, gamma=gamma)
        P, w, b, _, _ = R.fit(*args, **kw)
        Ps, ws, bs, _, _ = R.fit(*args, slow=True, **kw)
        tag = (degree, fit_lower, fit_linear, fit_intercept, gamma)
        assert abs(b - bs) < 1e-7, tag
        np.testing.assert_allclose(w, ws, rtol=1e-6, atol=1e-9, err_msg=str(tag))
        np.testing.assert_allclose(P, Ps, rtol=1e-6, atol=1e-9, err_msg=str(tag))


def test_eval_is_the_anova_polynomial_of_the_row_norms():
    Po = np.random.default_rng(3).standard_normal((7, 3))
    norms = np.sqrt((Po ** 2).sum(1))
    for deg in (1, 2, 3, 4):
        want = sum(np.prod(norms[list(c)]) for c in itertools.combinations(range(7), deg))
        np.testing.assert_allclose(R.eval_omegacs(Po.tolist(), deg), want, rtol=1e-13)


# ---------------------------------------------------------------- (b) the run order
def _same(a, b):
    """P, w, the intercept and viol bit for bit; the running loss total is summed in the order of the walk"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and \
        [v for v, _ in a[3]] == [v for v, _ in b[3]] and np.allclose([l for _, l in a[3]], [l for _, l in b[3]], rtol=1e-10)


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", ["edges", "edges_gaps", "ui_30_40"])
def test_run_order_is_bit_equal(case, degree):
    Xo, y = data_of(case)
    kw = dict(maxIter=3, tol=0.0, gamma=GAMMA.get((case, degree, K, "explicit"), 1e-3), **FIT_KW.get(case, {}))
    fits = {o: restated(Xo, y, degree, "explicit", True, False, order=o, **kw) for o in ("reference", "run")}
    assert _same(fits["reference"], fits["run"])


def _fit_example(degree, order):
    indptr, indices, data, n, d = _example_012()
    y = np.array([1.0, -0.5, 2.0])
    P0 = np.array([[[0.3, -0.2, 0.4], [0.1, 0.5, -0.3]]])
    return R.fit(indptr, indices, data, y, P0, np.zeros(d), 0.0, degree, 0, False, False, maxIter=2, tol=0.0, beta=1e-3, gamma=0.05,
                 order=order)


def test_level_order_differs_on_the_three_column_example():
    """DESIGN.md section 13's example: level order 0, 2, 1 against the chain's 0, 1, 2"""
    for degree in (2, 3):
        assert _same(_fit_example(degree, "reference"), _fit_example(degree, "run"))
    assert not np.array_equal(_fit_example(2, "reference")[0], _fit_example(2, "level")[0])


# ---------------------------------------------------------------- (c) both recompute branches
@pytest.mark.parametrize("degree", [2, 3])
def test_both_recompute_branches_are_taken(degree):
    """the reference's strong-regularisation strengths (tests/test_pbcd_omegacs.nim:190-193): the rows collapse, the
    polynomials without row j and the running ones fall below 0 by rounding and are computed afresh"""
    Xo, _, y = make_fm_dataset(N, D, degree, K, RECOMPUTE_SEEDS[degree], "explicit", True, True, scale=1.0)
    for order in ("reference", "run"):
        restated(Xo, y, degree, "explicit", True, False, order=order, maxIter=5, tol=0.0, alpha0=1e5, alpha=1e5, beta=1e5,
                 gamma=1e5)
        assert R.last_prox_recomputes > 0 and R.last_update_recomputes > 0, (order, R.last_prox_recomputes, R.last_update_recomputes)


# ---------------------------------------------------------------- (d) the gammas of the device file
def zero_row_share(P):
    """the share of all-zero rows of P [nOrders][k][d + nAug], over all orders together"""
    return float((P == 0.0).all(axis=1).mean())


@pytest.mark.parametrize("case,degree,k,fit_lower", list(GAMMA))
def test_gamma_zeroes_some_rows_and_not_all(case, degree, k, fit_lower):
    Xo, y = data_of(case)
    P = restated(Xo, y, degree, fit_lower, True, False, k=k, order="run", maxIter=ITERS[case], tol=0.0,
                 gamma=GAMMA[case, degree, k, fit_lower], **FIT_KW.get(case, {}))[0]
    share = zero_row_share(P)
    print("zero rows: %.1f %%" % (100 * share))
    assert 0.05 <= share <= 0.95, share


# ---------------------------------------------------------------- (e) refusals
def test_refusals_and_degrees():
    args = ([0, 1], [0], [1.0], [1.0])
    for degree in (2, 3, 4):
        R.fit(*args, np.zeros((1, 2, 1)), np.zeros(1), 0.0, degree, 0, False, False, maxIter=1)
    with pytest.raises(ValueError, match="no transpose"):
        R.fit(*args, np.zeros((1, 2, 1)), np.zeros(1), 0.0, 2, 0, False, False, transpose=True)
