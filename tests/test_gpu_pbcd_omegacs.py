"""-m gpu: proximal block coordinate descent with the OmegaCS regulariser (newPBCD(reg=newOmegaCS()), optimizer/pbcd.nim at
maxSearch = 0 with regularizer/omegacs.nim:31-85) on the device, against the plain-Python restatement of the reference's loop
and hooks (tests/pbcd_omegacs_restatement.py), walked in the reference's order (ascending j).

OmegaCS runs the run schedule at every degree, its cache and dcache resident on the device for the whole fit.  Tolerances
as PBCD's: with squared loss, no intercept and no dummy features P, w and viol are BIT-equal to the restatement; the
intercept's and the loss's sums over all samples are a fixed tree on the device (the reference keeps a running loss total;
the dummy features' sums are in the reference's order for OmegaCS): 1e-10 relative there.  Every gamma comes from tests/test_pbcd_omegacs_restatement.py's table, which that
file holds to zeroing between 5 % and 95 % of the rows."""
import ctypes as _C
import itertools

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
from common import make_fm_dataset, random_csr
import cd_schedule_cases as S
import pbcd_omegacs_restatement as R
from pbcd_omegacs_direct_child import compare as compare_direct_launches
from test_gpu_cd import Csr, csr_of
from test_pbcd_omegacs_restatement import FIT_KW, GAMMA, ITERS, RECOMPUTE_SEEDS, data_of, zero_row_share

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
N, D, K = 50, 6, 4
SUITE = list(itertools.product((2, 3, 4), ("explicit", "none", "augment")))


def device_fit(X, y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, task="regression", **kw):
    fm = nf.newFactorizationMachine(task, degree=degree, nComponents=P0.shape[1], fitLower=fit_lower, fitLinear=fit_linear,
                                    fitIntercept=fit_intercept, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = nf.newPBCD(verbose=0, reg=nf.newOmegaCS(), **kw)
    opt.fit(X, y, fm)
    return fm, opt


def check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, k=K, task="regression", seed=1, exact=False, **kw):
    P0, w0, b0, n_aug = S.start(Xo, degree, k, fit_lower, fit_linear, fit_intercept, seed=seed)
    fm, opt = device_fit(csr_of(Xo), y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, task=task, **kw)
    P, w, b, hist, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept, task=task,
                             **kw)
    tag = "omegacs deg %d %s lin %s icpt %s k %d %s" % (degree, fit_lower, fit_linear, fit_intercept, k, kw)
    assert len(opt.history) == len(hist), tag
    if exact:
        assert np.array_equal(fm.P, P), tag
        assert np.array_equal(fm.w, w), tag
        assert [v for v, _ in opt.history] == [v for v, _ in hist], tag
    np.testing.assert_allclose(fm.P, P, rtol=RTOL, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(fm.w, w, rtol=RTOL, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(fm.intercept, b, rtol=RTOL, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(np.array(opt.history), np.array(hist), rtol=RTOL, atol=ATOL, err_msg=tag)
    return fm, opt, P


def check_case(case, degree, fit_lower, fit_linear, fit_intercept, k=K, **kw):
    """a named input of tests/test_pbcd_omegacs_restatement.py at its sized gamma and its own strengths"""
    Xo, y = data_of(case)
    args = dict(maxIter=ITERS[case], tol=0.0, gamma=GAMMA[case, degree, k, fit_lower], **FIT_KW.get(case, {}))
    args.update(kw)
    return check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, k=k, **args)


def grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.3):
    Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=threshold)
    return Xo, y


def new_fm(degree, fit_lower, fit_linear, fit_intercept, **kw):
    return nf.newFactorizationMachine("regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                                      fitIntercept=fit_intercept, randomState=1, **kw)


def new_opt(**kw):
    return nf.newPBCD(verbose=0, tol=0, reg=nf.newOmegaCS(), **kw)


# ---------------------------------------------------------------- the reference's own suite (tests/test_pbcd_omegacs.nim)
@pytest.mark.parametrize("degree,fit_lower", SUITE)
def test_reference_suite(degree, fit_lower):
    for fit_intercept in (True, False):  # fitLinear = false leaves w at 0
        Xo, y = grid_data(degree, fit_lower, False, fit_intercept, threshold=0.0)
        fm = new_fm(degree, fit_lower, False, fit_intercept)
        new_opt(maxIter=10).fit(csr_of(Xo), y, fm)
        assert np.all(fm.w == 0.0)
    for fit_linear in (True, False):  # fitIntercept = false leaves the intercept at 0
        Xo, y = grid_data(degree, fit_lower, fit_linear, False, threshold=0.0)
        fm = new_fm(degree, fit_lower, fit_linear, False)
        new_opt(maxIter=10).fit(csr_of(Xo), y, fm)
        assert fm.intercept == 0.0
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.0)
        X = csr_of(Xo)
        warm = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)  # warm start
        opt = new_opt(maxIter=1)
        for _ in range(10):
            opt.fit(X, y, warm)
        cold = new_fm(degree, fit_lower, fit_linear, fit_intercept)
        new_opt(maxIter=10).fit(X, y, cold)
        assert abs(cold.intercept - warm.intercept) < 1e-8
        np.testing.assert_allclose(cold.w, warm.w, atol=1e-8, rtol=0)
        np.testing.assert_allclose(cold.P, warm.P, atol=1e-8, rtol=0)
        fm = new_fm(degree, fit_lower, fit_linear, fit_intercept)  # the score decreases
        fm.init(X)
        before = fm.score(X, y)
        new_opt(maxIter=20, alpha0=1e-9, alpha=1e-9, beta=1e-9, gamma=1e-9).fit(X, y, fm)
        assert fm.score(X, y) < before
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):  # strong vs weak regularisation
        Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, scale=3.0)
        X = csr_of(Xo)
        weak = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        strong = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        new_opt(maxIter=100, alpha0=0, alpha=0, beta=0, gamma=0).fit(X, y, weak)
        new_opt(maxIter=100, alpha0=1e5, alpha=1e5, beta=1e5, gamma=1e5).fit(X, y, strong)
        assert weak.score(X, y) < strong.score(X, y)
        assert abs(weak.intercept) >= abs(strong.intercept)
        assert np.linalg.norm(weak.w) >= np.linalg.norm(strong.w)
        assert np.linalg.norm(weak.P) >= np.linalg.norm(strong.P)


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("fit_linear,fit_intercept", list(itertools.product((True, False), (True, False))))
@pytest.mark.parametrize("degree,fit_lower", SUITE)
def test_parity_grid(degree, fit_lower, fit_linear, fit_intercept):
    """[4-augment-False-True] (degree 4, one dummy feature, no w, intercept) is the ill-conditioned one: the restatement
    alone moves by 4.3e-11 in P and 1.6e-10 in the third iteration's viol when the intercept's and the dummy feature's sums
    over the samples are associated as the device's 1024-leaf tree, and by 3.7e-15 and 0 with the tree for the intercept
    alone.  k_pb_dummy forms the dummy feature's sums in the reference's order for OmegaCS, which holds this case inside
    the bound."""
    Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept)
    check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, maxIter=3, tol=0.0, gamma=1e-3)


@pytest.mark.parametrize("loss,task", [("squared", "regression"), ("huber", "regression"), ("squared_hinge", "classification"),
                                       ("logistic", "classification")])
def test_parity_losses(loss, task):
    for degree, iters in ((2, 4), (3, 3)):
        Xo, y = grid_data(degree, "explicit", True, True)
        check_parity(Xo, y, degree, "explicit", True, True, task=task, maxIter=iters, tol=0.0, gamma=1e-3, loss=loss)


@pytest.mark.parametrize("degree", [2, 3])
def test_bit_equal_to_the_reference_order(degree):
    for Xo, y in (grid_data(degree, "explicit", True, False), data_of("ui_30_40")):
        for fit_linear in (True, False):
            check_parity(Xo, y, degree, "explicit", fit_linear, False, exact=True, maxIter=4, tol=0.0, gamma=1e-3)


# ---------------------------------------------------------------- the schedule
def device_schedule(Xo):
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    fm.init(csr_of(Xo))
    return nf.newPBCD(verbose=0, reg=nf.newOmegaCS()).schedule(csr_of(Xo), fm)


def test_schedule_reports_runs():
    Xo = Csr([0, 2, 3, 4], [0, 1, 1, 2], [1.0, 0.5, -0.7, 1.3], 3, 3)  # the three-column example of DESIGN.md section 13
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=2, fitLinear=False, fitIntercept=False)
    fm.init(csr_of(Xo))
    assert nf.newPBCD(verbose=0, reg=nf.newOmegaCS()).schedule(csr_of(Xo), fm) == (2, 2)  # runs [0], [1, 2]
    for degree in (2, 3):
        check_parity(Xo, np.array([1.0, -0.5, 2.0]), degree, "explicit", False, False, k=2, exact=True, maxIter=3, tol=0.0,
                     beta=1e-3, gamma=0.05)
    assert device_schedule(data_of("ui_60_80")[0]) == (2, 80)  # the users, then the items


@pytest.mark.parametrize("degree", [2, 3])
def test_schedule_edges_bit_equal(degree):
    """runs of 63, 64, 65, 1, 16, 17, 15, 130 and 5 features: k_pb_sq_runs three times per sweep, twice behind a wide run's
    three launches; columns of 63, 64, 65, 1, 129 and 322 entries"""
    assert device_schedule(data_of("edges")[0]) == (9, 130)
    for fit_linear in (True, False):
        check_case("edges", degree, "explicit", fit_linear, False, exact=True)


@pytest.mark.parametrize("k", S.PBCD_K)
def test_schedule_edges_components(k):
    """pb_grad's two layouts and the chain's norm over k components: k = 3, 5, 32, 33, 64, 65"""
    check_case("edges", 2, "explicit", True, False, k=k, exact=True)
    if k in (3, 33):
        check_case("edges", 3, "explicit", True, False, k=k, exact=True, maxIter=2)


def test_schedule_edges_behind_empty_columns():
    """beta = alpha = 0 with an unused id behind every feature: an empty column's invStepSize is clamped to 1e-12
    (pbcd.nim:148), so lam = gamma / 1e-12 and the prox takes the row to zero; everything stays finite"""
    Xo, _ = data_of("edges_gaps")
    assert device_schedule(Xo) == (10, 130)
    fm, opt, _ = check_case("edges_gaps", 2, "explicit", True, False, exact=True)
    assert np.isfinite(fm.P).all() and np.isfinite(fm.w).all() and np.isfinite(np.array(opt.history)).all()
    assert np.all(fm.P[:, :, S.empty_columns("edges_gaps")] == 0.0)
    check_case("edges_gaps", 2, "explicit", True, True)


def test_schedule_long_sums_over_every_sample():
    """n = 2050: k_cd_intercept, k_pb_dummy and k_cd_loss take two full trips of their 1024 threads and a partial one; at degree
    3 with augment the dummy feature continues OmegaCS's chain through k_pb_dummy"""
    check_case("long_1025", 2, "explicit", True, True, k=5)
    check_case("long_1025", 3, "augment", True, True, k=5)


def test_schedule_long_wide_run_with_two_blocks_of_components():
    assert device_schedule(data_of("long_1025")[0]) == (4, 1025)
    check_case("long_1025", 2, "explicit", True, False, k=65, exact=True)


def test_wide_runs_at_degree_3():
    """user x item with 80 items: the item run is a launch of its own (k_pb_sq_pre / k_pb_sq_chain / k_pb_sq_post) at degree
    3, a path SquaredL21 (degree 2 only) never takes"""
    check_case("ui_60_80", 2, "explicit", True, False, exact=True)
    check_case("ui_60_80", 3, "explicit", True, False, exact=True)
    check_case("ui_60_80", 3, "augment", True, True)


@pytest.mark.parametrize("degree", [2, 3])
def test_both_recompute_branches(degree):
    """omegacs.nim:71-79 and :60-61 on the inputs tests/test_pbcd_omegacs_restatement.py shows taking them"""
    Xo, _, y = make_fm_dataset(N, D, degree, K, RECOMPUTE_SEEDS[degree], "explicit", True, True, scale=1.0)
    strong = dict(maxIter=5, tol=0.0, alpha0=1e5, alpha=1e5, beta=1e5, gamma=1e5)
    check_parity(Xo, y, degree, "explicit", True, False, exact=True, **strong)
    assert R.last_prox_recomputes > 0 and R.last_update_recomputes > 0
    check_parity(Xo, y, degree, "explicit", True, True, **strong)
    assert R.last_prox_recomputes > 0 and R.last_update_recomputes > 0


@pytest.mark.parametrize("k", [1, 130])
def test_components(k):
    check_case("ui_40_50", 2, "explicit", True, True, k=k)


def test_zero_pattern():
    """OmegaCS selects features: a row of P is zero as a whole or not at all"""
    fm, _, _ = check_case("edges", 2, "explicit", True, False, exact=True)
    zero_rows = (fm.P[0] == 0.0).all(axis=0)
    assert zero_rows.any() and not zero_rows.all()
    assert np.array_equal((fm.P[0] == 0.0).any(axis=0), zero_rows)
    assert 0.05 <= zero_row_share(fm.P) <= 0.95


def test_ml100k_shape():
    """943 users x 1682 items one-hot, 100 000 pairs, k = 4, 2 iterations"""
    check_case("ml100k", 2, "explicit", True, True)


def test_direct_launches_equal_the_graph(tmp_path):
    compare_direct_launches(3, tmp_path)


# ---------------------------------------------------------------- errors
def test_errors():
    L = capi.lib()
    Xo = random_csr(30, 10, 3, seed=1, sorted_idx=True)
    X = csr_of(Xo)
    args = (1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0)
    reg = capi.REG["omegacs"]
    for degree in (2, 3):
        fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=3)
        fm.init(X)
        h = _C.c_void_p()
        assert L.nfm_pbcd_create(fm._push(X.ctx), *args, reg, 0, _C.byref(h)) == 0
        L.nfm_opt_destroy(h)
        h = _C.c_void_p()
        assert L.nfm_pbcd_create(fm._push(X.ctx), *args, reg, 2, _C.byref(h)) == capi.ERR_UNSUPPORTED  # max_search
        h = _C.c_void_p()
        assert L.nfm_pcd_create(fm._push(X.ctx), *args, reg, 0, _C.byref(h)) == capi.ERR_UNSUPPORTED
        assert b"OmegaCS" in L.nfm_last_error()
        h = _C.c_void_p()
        assert L.nfm_pgd_create(fm._push(X.ctx), 0, 1e-6, 1e-3, 1e-4, 1e-4, 0.5, 0.01, 1.0, 0, 1.0, reg, 0, 10,
                                _C.byref(h)) == capi.ERR_UNSUPPORTED
        assert b"OmegaCS" in L.nfm_last_error()
        h = _C.c_void_p()
        assert L.nfm_pbcd_create(fm._push(X.ctx), *args, 7, 0, _C.byref(h)) == capi.ERR_INVALID
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)  # a field-aware model
    Xf = nf.newCSRFieldDataset(np.ones(4), np.array([0, 1, 2, 3]), np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2, 4, 2)
    ffm.init(Xf)
    hf = _C.c_void_p()
    assert L.nfm_pbcd_create(ffm._push(Xf.ctx), *args, reg, 0, _C.byref(hf)) == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        nf.newPBCD(verbose=0, maxIter=1, reg=nf.newOmegaCS()).fit(Xf, np.ones(2), ffm)
    for make in (nf.newPCD, nf.newPGD, nf.newFISTA, nf.newNMAPGD, nf.newKatyusha, nf.newMBPSGD):
        with pytest.raises(ValueError):
            make(reg=nf.newOmegaCS())
    with pytest.raises(ValueError, match="maxSearch"):
        nf.newPBCD(reg=nf.newOmegaCS(), maxSearch=3)
    with pytest.raises(ValueError, match=r"newOmegaCS\(\)"):
        nf.newPBCD(reg=nf.newOmegaTI())


def test_verbose_line_penalty():
    """pbcd.nim:303-306 with the unscaled strengths: gamma times the ANOVA polynomial of the row norms, per order"""
    Xo, y = grid_data(3, "explicit", True, True)
    fm = nf.newFactorizationMachine("regression", degree=3, nComponents=K)
    opt = nf.newPBCD(maxIter=1, tol=0.0, verbose=0, reg=nf.newOmegaCS(), gamma=1e-3)
    opt.fit(csr_of(Xo), y, fm)
    want = 0.5 * opt.alpha0 * fm.intercept ** 2 + 0.5 * opt.alpha * (fm.w ** 2).sum() + 0.5 * opt.beta * (fm.P ** 2).sum()
    for order in range(fm.P.shape[0]):
        norms = np.sqrt((fm.P[order] ** 2).sum(0))
        want += opt.gamma * sum(np.prod(norms[list(c)]) for c in itertools.combinations(range(len(norms)), 3 - order))
    np.testing.assert_allclose(opt._penalty(fm, 50.0) / 50.0, want, rtol=1e-12)
