"""-m gpu: coordinate descent (newCD, optimizer/cd.nim) on the device -- nfm_cd_create / nfm_cd_begin_fit / nfm_opt_epoch --
against the plain-Python restatement of the reference's loop (tests/cd_restatement.py).

Tolerances: the features of the rows run in the level schedule with every sum in the reference's order, so with squared
loss, no intercept and no dummy features the parameters and viol are BIT-equal to the restatement.  The intercept's and the
dummy features' sums over all samples are a fixed tree on the device, and the loss sum likewise: 1e-10 relative there."""
import itertools

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
from common import init_fm, make_fm_dataset, random_csr
import cd_restatement as R
import cd_schedule_cases as S
from cd_direct_child import compare as compare_direct_launches

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
N, D, K = 50, 6, 4
GRID = list(itertools.product((2, 3, 4), ("explicit", "none", "augment"), (True, False), (True, False)))


def csr_of(Xo):
    return nf.newCSRDataset(Xo.data, Xo.indices, Xo.indptr, Xo.n, Xo.d)


def device_fit(X, y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, task="regression", **cd):
    k = P0.shape[1]
    fm = nf.newFactorizationMachine(task, degree=degree, nComponents=k, fitLower=fit_lower, fitLinear=fit_linear,
                                    fitIntercept=fit_intercept, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = nf.newCD(verbose=0, **cd)
    opt.fit(X, y, fm)
    return fm, opt


def restated(indptr, indices, data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, task="regression", **cd):
    cd = dict(cd)
    return R.fit(indptr, indices, data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, task=task, **cd)


def close(a, b, what):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=what)


def check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, k=K, task="regression", seed=1, exact=False, **cd):
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fit_linear, seed=seed, scale=0.1)
    w0 = np.random.default_rng(seed + 5).uniform(-0.1, 0.1, Xo.d) if fit_linear else w0
    b0 = 0.05 if fit_intercept else 0.0
    fm, opt = device_fit(csr_of(Xo), y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, task=task, **cd)
    P, w, b, hist, _ = restated(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                                task=task, **cd)
    tag = "deg %d %s lin %s icpt %s %s" % (degree, fit_lower, fit_linear, fit_intercept, cd)
    assert len(opt.history) == len(hist), tag
    if exact:
        assert np.array_equal(fm.P, P), tag
        assert np.array_equal(fm.w, w), tag
        assert [v for v, _ in opt.history] == [v for v, _ in hist], tag
    close(fm.P, P, tag)
    close(fm.w, w, tag)
    close(fm.intercept, b, tag)
    close(np.array(opt.history), np.array(hist), tag)
    return fm, opt


def grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.3):
    Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=threshold)
    return Xo, y


# ---------------------------------------------------------------- the reference's own tests (tests/test_cd.nim)
@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_fit_linear_false_leaves_w_zero(degree, fit_lower):
    for fit_intercept in (True, False):
        Xo, y = grid_data(degree, fit_lower, False, fit_intercept, threshold=0.0)
        fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=False,
                                        fitIntercept=fit_intercept, randomState=1)
        nf.newCD(maxIter=10, verbose=0, tol=0).fit(csr_of(Xo), y, fm)
        assert np.all(fm.w == 0.0)


@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_fit_intercept_false_leaves_b_zero(degree, fit_lower):
    for fit_linear in (True, False):
        Xo, y = grid_data(degree, fit_lower, fit_linear, False, threshold=0.0)
        fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                                        fitIntercept=False, randomState=1)
        nf.newCD(maxIter=10, verbose=0, tol=0).fit(csr_of(Xo), y, fm)
        assert fm.intercept == 0.0


@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_warm_start(degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.0)
        X = csr_of(Xo)
        kw = dict(task="regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                  fitIntercept=fit_intercept, randomState=1)
        warm = nf.newFactorizationMachine(warmStart=True, **kw)
        cd_warm = nf.newCD(maxIter=1, verbose=0, tol=0)
        for _ in range(10):
            cd_warm.fit(X, y, warm)
        cold = nf.newFactorizationMachine(**kw)
        nf.newCD(maxIter=10, verbose=0, tol=0).fit(X, y, cold)
        assert abs(cold.intercept - warm.intercept) < 1e-8
        np.testing.assert_allclose(cold.w, warm.w, atol=1e-8, rtol=0)
        np.testing.assert_allclose(cold.P, warm.P, atol=1e-8, rtol=0)


@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_score_decreases(degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.0)
        X = csr_of(Xo)
        fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                                        fitIntercept=fit_intercept, randomState=1)
        fm.init(X)
        before = fm.score(X, y)
        nf.newCD(maxIter=20, verbose=0, tol=0, alpha0=1e-9, alpha=1e-9, beta=1e-9).fit(X, y, fm)
        assert fm.score(X, y) < before


@pytest.mark.parametrize("degree,fit_lower", list(itertools.product((2, 3, 4), ("explicit", "none", "augment"))))
def test_regularization(degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, scale=1.0)
        X = csr_of(Xo)
        kw = dict(task="regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                  fitIntercept=fit_intercept, randomState=1, warmStart=True)
        weak, strong = nf.newFactorizationMachine(**kw), nf.newFactorizationMachine(**kw)
        nf.newCD(maxIter=100, verbose=0, tol=0, alpha0=0, alpha=0, beta=0).fit(X, y, weak)
        nf.newCD(maxIter=100, verbose=0, tol=0, alpha0=1e6, alpha=1e6, beta=1e6).fit(X, y, strong)
        assert weak.score(X, y) < strong.score(X, y)
        assert abs(weak.intercept) >= abs(strong.intercept)
        assert np.linalg.norm(weak.w) >= np.linalg.norm(strong.w)
        assert np.linalg.norm(weak.P) >= np.linalg.norm(strong.P)


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("degree,fit_lower,fit_linear,fit_intercept", GRID)
def test_parity_grid(degree, fit_lower, fit_linear, fit_intercept):
    Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept)
    check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, maxIter=3, tol=0.0)


@pytest.mark.parametrize("loss", ["squared", "squared_hinge", "logistic", "huber"])
@pytest.mark.parametrize("task", ["regression", "classification"])
def test_parity_losses(loss, task):
    for degree, fit_lower in ((2, "explicit"), (3, "explicit"), (3, "augment")):
        Xo, y = grid_data(degree, fit_lower, True, True)
        check_parity(Xo, y, degree, fit_lower, True, True, task=task, maxIter=4, tol=0.0, loss=loss, lossParam=0.3,
                     alpha0=1e-4, alpha=1e-3, beta=1e-3)


def test_history_stops_where_the_restatement_stops():
    Xo, y = grid_data(2, "explicit", True, True)
    P0, w0, b0, n_aug = init_fm(Xo.d, 2, K, "explicit", True, seed=1, scale=0.1)
    w0 = np.random.default_rng(6).uniform(-0.1, 0.1, Xo.d)
    hist = restated(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, 0.05, 2, n_aug, True, True, maxIter=30, tol=0.0)[3]
    tol = hist[9][0] * (1 + 1e-9)  # stops at the 10th iteration at the latest
    fm, opt = check_parity(Xo, y, 2, "explicit", True, True, maxIter=30, tol=tol)
    assert 1 < len(opt.history) <= 10


@pytest.mark.parametrize("degree", [2, 3])
def test_bit_equal_to_the_reference_order(degree):
    """squared loss, no intercept, sorted rows, explicit lower orders: every sum of the device is the reference's"""
    Xo = random_csr(300, 40, 9, seed=degree, sorted_idx=True)
    y = np.random.default_rng(3).standard_normal(Xo.n)
    for fit_linear in (True, False):
        check_parity(Xo, y, degree, "explicit", fit_linear, False, exact=True, maxIter=4, tol=0.0)


# ---------------------------------------------------------------- shapes
class Csr:
    def __init__(self, indptr, indices, data, n, d):
        self.indptr, self.indices, self.data, self.n, self.d = (np.asarray(indptr, np.int64), np.asarray(indices, np.int64),
                                                                np.asarray(data, np.float64), n, d)


def user_item(n_users, n_items, n, seed, skew=1.1):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users, n)
    pop = 1.0 / np.arange(1, n_items + 1) ** skew
    it = rng.choice(n_items, n, p=pop / pop.sum())
    pairs = np.unique(np.stack([u, it], 1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    m = len(pairs)
    # every user and item used once at least (so that no column is empty)
    extra_u = np.stack([np.arange(n_users), rng.integers(0, n_items, n_users)], 1)
    extra_i = np.stack([rng.integers(0, n_users, n_items), np.arange(n_items)], 1)
    pairs = np.concatenate([pairs, extra_u, extra_i])
    m = len(pairs)
    indices = np.stack([pairs[:, 0], n_users + pairs[:, 1]], 1).reshape(-1)
    y = rng.integers(1, 6, m).astype(np.float64)
    return Csr(np.arange(0, 2 * m + 1, 2), indices, np.ones(2 * m), m, n_users + n_items), y


def schedule(X, degree=2, k=K, fit_lower="explicit", fit_linear=True):
    fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=k, fitLower=fit_lower, fitLinear=fit_linear)
    fm.init(X)
    return nf.newCD(verbose=0).schedule(X, fm)


def test_user_item_has_two_levels():
    Xo, y = user_item(40, 60, 500, seed=1)
    assert schedule(csr_of(Xo)) == (2, 60)
    assert R.schedule_depth(Xo.indptr, Xo.indices, Xo.n, Xo.d) == (2, 60)
    check_parity(Xo, y, 2, "explicit", True, True, maxIter=3, tol=0.0)


def test_random_rows_deep_schedule():
    Xo = random_csr(400, 120, 32, seed=4, sorted_idx=True)
    y = np.random.default_rng(4).standard_normal(Xo.n)
    depth, widest = schedule(csr_of(Xo))
    assert depth > 10 and (depth, widest) == R.schedule_depth(Xo.indptr, Xo.indices, Xo.n, Xo.d)
    check_parity(Xo, y, 2, "explicit", True, False, exact=True, maxIter=2, tol=0.0)


def test_empty_rows_and_unused_features():
    rng = np.random.default_rng(5)
    n, d = 80, 30
    rows = [np.sort(rng.choice(20, rng.integers(0, 6), replace=False)) if i % 5 else np.zeros(0, np.int64) for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    Xo = Csr(indptr, np.concatenate(rows), rng.uniform(-1, 1, indptr[-1]), n, d)  # features 20 .. 29 unused
    y = rng.standard_normal(n)
    # degree 2 and the linear term skip a step whose invStepSize < 1e-12 (cd.nim:99-100, fit_linear.nim:20-21): an unused feature
    # with beta = alpha = 0; the general epoch has no such guard (0 / 0 there), so degree 3 keeps beta > 0
    check_parity(Xo, y, 2, "explicit", True, True, maxIter=3, tol=0.0, beta=0.0, alpha=0.0)
    check_parity(Xo, y, 3, "explicit", True, True, maxIter=3, tol=0.0)


def test_unsorted_rows():
    Xo = random_csr(200, 50, 12, seed=6, sorted_idx=False)
    assert any(np.any(np.diff(Xo.indices[Xo.indptr[i]:Xo.indptr[i + 1]]) < 0) for i in range(Xo.n))
    y = np.random.default_rng(6).standard_normal(Xo.n)
    for degree in (2, 3):
        check_parity(Xo, y, degree, "explicit", True, False, exact=True, maxIter=3, tol=0.0)


def test_feature_in_every_sample():
    Xo = random_csr(150, 30, 6, seed=7, sorted_idx=True)
    rows = []
    for i in range(Xo.n):
        idx = Xo.indices[Xo.indptr[i]:Xo.indptr[i + 1]]
        val = Xo.data[Xo.indptr[i]:Xo.indptr[i + 1]]
        keep = idx != 0
        rows.append((np.concatenate([[0], idx[keep]]), np.concatenate([[0.7], val[keep]])))
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
    Xa = Csr(indptr, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), Xo.n, Xo.d)
    y = np.random.default_rng(7).standard_normal(Xa.n)
    check_parity(Xa, y, 2, "explicit", True, True, maxIter=3, tol=0.0)
    check_parity(Xa, y, 3, "explicit", True, False, exact=True, maxIter=3, tol=0.0)


@pytest.mark.parametrize("degree", [3, 4])
def test_augment(degree):
    Xo = random_csr(120, 25, 7, seed=degree, sorted_idx=True)
    y = np.random.default_rng(8).standard_normal(Xo.n)
    for fit_linear in (True, False):
        check_parity(Xo, y, degree, "augment", fit_linear, True, maxIter=3, tol=0.0)


@pytest.mark.parametrize("k", [1, 130])
def test_components(k):
    Xo = random_csr(60, 20, 5, seed=k, sorted_idx=True)
    y = np.random.default_rng(k).standard_normal(Xo.n)
    check_parity(Xo, y, 2, "explicit", True, True, k=k, maxIter=2, tol=0.0)
    check_parity(Xo, y, 3, "explicit", True, False, k=k, exact=True, maxIter=2, tol=0.0)


def test_ml100k_shape():
    """943 users x 1682 items one-hot, 100 000 pairs with skewed item popularity, k = 4: 3 iterations"""
    Xo, y = user_item(943, 1682, 100000, seed=11)
    assert schedule(csr_of(Xo))[0] == 2
    check_parity(Xo, y, 2, "explicit", True, True, maxIter=3, tol=0.0, alpha0=1e-7, alpha=1e-5, beta=1e-3)


# ---------------------------------------------------------------- the schedule's edges (tests/cd_schedule_cases.py)
@pytest.mark.parametrize("degree", [2, 3])
def test_schedule_edges_bit_equal(degree):
    """levels of 63, 64, 65, 1, 16, 17, 15, 130 and 5 features: k_cd_levels, k_cd_level twice, k_cd_levels from g0 = 3,
    k_cd_level, k_cd_levels; columns of 63, 64, 65, 1, 129 and 322 entries"""
    Xo, y = S.inputs("edges")
    assert schedule(csr_of(Xo)) == R.schedule_depth(Xo.indptr, Xo.indices, Xo.n, Xo.d) == (9, 130)
    for fit_linear in (True, False):
        check_parity(Xo, y, degree, "explicit", fit_linear, False, exact=True, maxIter=3, tol=0.0)


def test_schedule_edges_intercept_and_logistic():
    Xo, y = S.inputs("edges")
    check_parity(Xo, y, 3, "explicit", True, True, task="classification", loss="logistic", maxIter=3, tol=0.0)


def test_schedule_edges_behind_empty_columns():
    """every feature followed by an unused id: level 0 is a wide launch of 331 skipped steps at beta = alpha = 0 (degree 2 and
    the linear term; the general epoch has no guard, so degree 3 keeps beta > 0, as test_empty_rows_and_unused_features says)"""
    Xo, y = S.inputs("edges_gaps")
    assert schedule(csr_of(Xo)) == R.schedule_depth(Xo.indptr, Xo.indices, Xo.n, Xo.d) == (11, 331)
    empty = S.empty_columns("edges_gaps")
    for fit_linear in (True, False):
        fm, _ = check_parity(Xo, y, 2, "explicit", fit_linear, False, exact=True, maxIter=3, tol=0.0, beta=0.0, alpha=0.0)
        P0, w0, _, _ = S.start(Xo, 2, K, "explicit", fit_linear, False)
        assert np.array_equal(fm.P[:, :, empty], P0[:, :, empty]) and np.array_equal(fm.w[empty], w0[empty])
        assert np.isfinite(fm.P).all() and np.isfinite(fm.w).all()
    check_parity(Xo, y, 3, "explicit", True, False, exact=True, maxIter=3, tol=0.0)


def test_schedule_long_sums_over_every_sample():
    """n = 2050: k_cd_intercept, k_cd_dummy and k_cd_loss take two full trips of their 1024 threads and a partial one"""
    Xo, y = S.inputs("long_1025")
    check_parity(Xo, y, 3, "augment", True, True, task="classification", loss="logistic", maxIter=2, tol=0.0)


def test_direct_launches_equal_the_graph(tmp_path):
    compare_direct_launches("cd", None, 2, tmp_path)


# ---------------------------------------------------------------- errors
def _opt(fm, X):
    h = C_void()
    capi.check(capi.lib().nfm_cd_create(fm._push(X.ctx), 1e-6, 1e-3, 1e-3, 0, 1.0, C_byref(h)))
    return h


import ctypes as _C  # noqa: E402

C_void, C_byref = _C.c_void_p, _C.byref


def test_errors():
    L = capi.lib()
    Xo = random_csr(30, 10, 3, seed=1, sorted_idx=True)
    X = csr_of(Xo)
    X.set_targets(np.ones(X.nSamples))
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3)
    fm.init(X)
    h = _opt(fm, X)
    try:
        ls, vs = _C.c_double(), _C.c_double()
        assert L.nfm_opt_epoch(h, X.h, None, 0, X.nSamples, _C.byref(ls), _C.byref(vs)) == capi.ERR_INVALID  # before begin_fit
        assert L.nfm_cd_begin_fit(h, X.h) == 0
        perm = np.arange(X.nSamples, dtype=np.int64)
        assert L.nfm_opt_epoch(h, X.h, perm.ctypes.data_as(_C.c_void_p), 0, X.nSamples, _C.byref(ls), _C.byref(vs)) == capi.ERR_INVALID
        assert L.nfm_opt_epoch(h, X.h, None, 0, X.nSamples - 1, _C.byref(ls), _C.byref(vs)) == capi.ERR_INVALID
        assert L.nfm_opt_set_shuffle(h, 3) == capi.ERR_UNSUPPORTED
        assert L.nfm_opt_set_touch_cap(h, 4.0) == capi.ERR_UNSUPPORTED
        assert L.nfm_opt_set_ada_cross(h, 0.1) == capi.ERR_UNSUPPORTED
        assert L.nfm_opt_epoch(h, X.h, None, 0, X.nSamples, _C.byref(ls), _C.byref(vs)) == 0
        assert L.nfm_opt_finalize(h) == 0
    finally:
        L.nfm_opt_destroy(h)
    # a repeated id inside a row
    Xr = nf.newCSRDataset(np.ones(4), np.array([1, 1, 2, 3]), np.array([0, 2, 4]), 2, 5)
    fm2 = nf.newFactorizationMachine("regression", degree=2, nComponents=2)
    with pytest.raises(nf.NfmError) as e:
        nf.newCD(verbose=0, maxIter=1).fit(Xr, np.ones(2), fm2)
    assert e.value.code == capi.ERR_UNSUPPORTED
    # a field-aware model
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)
    Xf = nf.newCSRFieldDataset(np.ones(4), np.array([0, 1, 2, 3]), np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2, 4, 2)
    ffm.init(Xf)
    hf = _C.c_void_p()
    assert L.nfm_cd_create(ffm._push(Xf.ctx), 1e-6, 1e-3, 1e-3, 0, 1.0, _C.byref(hf)) == capi.ERR_UNSUPPORTED
