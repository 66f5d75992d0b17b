"""-m gpu: proximal block coordinate descent (newPBCD, optimizer/pbcd.nim at maxSearch = 0) on the device -- nfm_pbcd_create /
nfm_cd_begin_fit / nfm_opt_epoch -- against the plain-Python restatement of the reference's loop (tests/pbcd_restatement.py).

L1 and L21 run CD's level schedule, SquaredL21 (the default) the run schedule.  Tolerances as CD's and PCD's: with squared
loss, no intercept and no dummy features P, w and viol are BIT-equal to the restatement in the reference's order; the
intercept's, the dummy features' and the loss's sums over all samples are a fixed tree on the device (the reference keeps a
running loss total): 1e-10 relative there."""
import ctypes as _C
import itertools

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
from common import init_fm, make_fm_dataset, random_csr
import cd_schedule_cases as S
import pbcd_restatement as R
from cd_direct_child import compare as compare_direct_launches
from test_gpu_cd import Csr, csr_of, user_item
from test_gpu_pcd import _cli, _files

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
N, D, K = 50, 6, 4
REGS = {"l1": lambda: nf.newL1(), "l21": lambda: nf.newL21(), "squaredl21": lambda: nf.newSquaredL21()}
RESUM_SEED = 45  # tests/test_pbcd_restatement.py::test_resum_branch_is_taken shows the branch on this input


def degrees_of(reg):
    return (2,) if reg == "squaredl21" else (2, 3, 4)


def device_fit(X, y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, reg, task="regression", **kw):
    fm = nf.newFactorizationMachine(task, degree=degree, nComponents=P0.shape[1], fitLower=fit_lower, fitLinear=fit_linear,
                                    fitIntercept=fit_intercept, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = nf.newPBCD(verbose=0, reg=REGS[reg](), **kw)
    opt.fit(X, y, fm)
    return fm, opt


def check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, reg, k=K, task="regression", seed=1, exact=False,
                 **kw):
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fit_linear, seed=seed, scale=0.1)
    w0 = np.random.default_rng(seed + 5).uniform(-0.1, 0.1, Xo.d) if fit_linear else w0
    b0 = 0.05 if fit_intercept else 0.0
    fm, opt = device_fit(csr_of(Xo), y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, reg, task=task, **kw)
    P, w, b, hist, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                             task=task, reg=reg, **kw)
    tag = "%s deg %d %s lin %s icpt %s %s" % (reg, degree, fit_lower, fit_linear, fit_intercept, kw)
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


def grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.3):
    Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, threshold=threshold)
    return Xo, y


def new_fm(degree, fit_lower, fit_linear, fit_intercept, **kw):
    return nf.newFactorizationMachine("regression", degree=degree, nComponents=K, fitLower=fit_lower, fitLinear=fit_linear,
                                      fitIntercept=fit_intercept, randomState=1, **kw)


SUITE = [(r, d, fl) for r in REGS for d in degrees_of(r) for fl in ("explicit", "none", "augment")]


# ---------------------------------------------------------------- the reference's own suites
# (tests/test_pbcd_l1.nim, test_pbcd_l21.nim, test_pbcd_squaredl21.nim)
@pytest.mark.parametrize("reg,degree,fit_lower", SUITE)
def test_reference_suite(reg, degree, fit_lower):
    for fit_intercept in (True, False):  # fitLinear = false leaves w at 0
        Xo, y = grid_data(degree, fit_lower, False, fit_intercept, threshold=0.0)
        fm = new_fm(degree, fit_lower, False, fit_intercept)
        nf.newPBCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(csr_of(Xo), y, fm)
        assert np.all(fm.w == 0.0)
    for fit_linear in (True, False):  # fitIntercept = false leaves the intercept at 0
        Xo, y = grid_data(degree, fit_lower, fit_linear, False, threshold=0.0)
        fm = new_fm(degree, fit_lower, fit_linear, False)
        nf.newPBCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(csr_of(Xo), y, fm)
        assert fm.intercept == 0.0
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.0)
        X = csr_of(Xo)
        warm = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)  # warm start
        opt = nf.newPBCD(maxIter=1, verbose=0, tol=0, reg=REGS[reg]())
        for _ in range(10):
            opt.fit(X, y, warm)
        cold = new_fm(degree, fit_lower, fit_linear, fit_intercept)
        nf.newPBCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(X, y, cold)
        assert abs(cold.intercept - warm.intercept) < 1e-8
        np.testing.assert_allclose(cold.w, warm.w, atol=1e-8, rtol=0)
        np.testing.assert_allclose(cold.P, warm.P, atol=1e-8, rtol=0)
        fm = new_fm(degree, fit_lower, fit_linear, fit_intercept)  # the score decreases
        fm.init(X)
        before = fm.score(X, y)
        nf.newPBCD(maxIter=20, verbose=0, tol=0, alpha0=1e-9, alpha=1e-9, beta=1e-9, gamma=1e-9, reg=REGS[reg]()).fit(X, y, fm)
        assert fm.score(X, y) < before
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):  # strong vs weak regularisation
        Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, scale=1.0)
        X = csr_of(Xo)
        weak = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        strong = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        nf.newPBCD(maxIter=100, verbose=0, tol=0, alpha0=0, alpha=0, beta=0, gamma=0, reg=REGS[reg]()).fit(X, y, weak)
        nf.newPBCD(maxIter=100, verbose=0, tol=0, alpha0=1e5, alpha=1e5, beta=1e5, gamma=1e5, reg=REGS[reg]()).fit(X, y, strong)
        assert weak.score(X, y) < strong.score(X, y)
        assert abs(weak.intercept) >= abs(strong.intercept)
        assert np.linalg.norm(weak.w) >= np.linalg.norm(strong.w)
        assert np.linalg.norm(weak.P) >= np.linalg.norm(strong.P)


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("reg,degree,fit_lower", SUITE)
def test_parity_grid(reg, degree, fit_lower):
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept)
        check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, reg, maxIter=3, tol=0.0, gamma=1e-3)


@pytest.mark.parametrize("reg", list(REGS))
@pytest.mark.parametrize("loss,task", [("squared", "regression"), ("huber", "regression"), ("squared_hinge", "classification"),
                                       ("logistic", "classification")])
def test_parity_losses(reg, loss, task):
    Xo, y = grid_data(2, "explicit", True, True)
    check_parity(Xo, y, 2, "explicit", True, True, reg, task=task, maxIter=4, tol=0.0, gamma=1e-3, loss=loss)
    if reg != "squaredl21":
        Xo, y = grid_data(3, "explicit", True, True)
        check_parity(Xo, y, 3, "explicit", True, True, reg, task=task, maxIter=3, tol=0.0, gamma=1e-3, loss=loss)


@pytest.mark.parametrize("reg", list(REGS))
def test_bit_equal_to_the_reference_order(reg):
    for degree in degrees_of(reg)[:2]:  # degree 2, and degree 3 where allowed
        for name, (Xo, y) in {"grid": grid_data(degree, "explicit", True, False),
                              "user_item": user_item(30, 40, 300, seed=3)}.items():
            for fit_linear in (True, False):
                check_parity(Xo, y, degree, "explicit", fit_linear, False, reg, exact=True, maxIter=4, tol=0.0, gamma=1e-3)


# ---------------------------------------------------------------- the schedules
def test_schedule_reports_runs_or_levels():
    Xo = Csr([0, 2, 3, 4], [0, 1, 1, 2], [1.0, 0.5, -0.7, 1.3], 3, 3)  # the three-column example of DESIGN.md section 13
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=2, fitLinear=False, fitIntercept=False)
    fm.init(csr_of(Xo))
    assert nf.newPBCD(verbose=0).schedule(csr_of(Xo), fm) == (2, 2)  # runs [0], [1, 2]
    assert nf.newPBCD(verbose=0, reg=nf.newL21()).schedule(csr_of(Xo), fm) == (2, 2)  # levels {0, 2}, {1}
    check_parity(Xo, np.array([1.0, -0.5, 2.0]), 2, "explicit", False, False, "squaredl21", k=2, exact=True, maxIter=3, tol=0.0,
                 beta=1e-3, gamma=0.05)
    Xu, _ = user_item(60, 80, 900, seed=5)
    fmu = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    fmu.init(csr_of(Xu))
    assert nf.newPBCD(verbose=0).schedule(csr_of(Xu), fmu) == (2, 80)  # the users, then the items
    for reg in ("l1", "l21"):
        assert nf.newPBCD(verbose=0, reg=REGS[reg]()).schedule(csr_of(Xu), fmu)[0] == 2  # levels
    Xr = random_csr(120, 60, 5, seed=8, sorted_idx=True)
    fmr = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    fmr.init(csr_of(Xr))
    from pcd_restatement import schedule
    assert nf.newPBCD(verbose=0).schedule(csr_of(Xr), fmr) == schedule(Xr.indptr, Xr.indices, Xr.n, Xr.d, True)
    assert nf.newPBCD(verbose=0, reg=nf.newL1()).schedule(csr_of(Xr), fmr) == schedule(Xr.indptr, Xr.indices, Xr.n, Xr.d, False)


def test_wide_levels_and_wide_runs():
    """user x item with 80 items: the item level (run) is >= 64 features, a launch of its own -- k_pb_level for L1 and L21,
    k_pb_sq_pre / k_pb_sq_chain / k_pb_sq_post for SquaredL21 -- at degree 2 and 3"""
    Xu, yu = user_item(60, 80, 900, seed=5)
    for reg in REGS:
        check_parity(Xu, yu, 2, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, gamma=1e-3)
        check_parity(Xu, yu, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)
    for reg in ("l1", "l21"):
        check_parity(Xu, yu, 3, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, gamma=1e-3)
        check_parity(Xu, yu, 3, "augment", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)


def test_zero_patterns():
    """gamma = 0.05: L1 zeroes single coordinates, L21 whole rows of P (columns of fm.P[order], [k][d])"""
    Xo, y = grid_data(2, "explicit", True, False)
    _, _, P = check_parity(Xo, y, 2, "explicit", True, False, "l1", exact=True, maxIter=5, tol=0.0, gamma=0.05)
    assert 0 < (P == 0.0).sum() < P.size
    fm, _, P = check_parity(Xo, y, 2, "explicit", True, False, "l21", exact=True, maxIter=10, tol=0.0, gamma=0.05)
    zero_rows = (fm.P[0] == 0.0).all(axis=0)
    assert zero_rows.any() and not zero_rows.all()
    assert np.array_equal((fm.P[0] == 0.0).any(axis=0), zero_rows)  # a row is zero as a whole or not at all


def test_resum_branch():
    """squaredl21.nim:37-38 on the input tests/test_pbcd_restatement.py shows taking it"""
    Xo, _, y = make_fm_dataset(N, D, 2, K, RESUM_SEED, "explicit", True, True, scale=1.0)
    check_parity(Xo, y, 2, "explicit", True, True, "squaredl21", maxIter=5, tol=0.0, alpha0=1e5, alpha=1e5, beta=1e5, gamma=1e5)
    assert R.last_resums > 0
    check_parity(Xo, y, 2, "explicit", True, False, "squaredl21", exact=True, maxIter=5, tol=0.0, alpha0=1e5, alpha=1e5,
                 beta=1e5, gamma=1e5)
    assert R.last_resums > 0


def test_empty_columns_and_unsorted_rows():
    Xo = random_csr(120, 60, 5, seed=8, sorted_idx=False)
    X = Csr(Xo.indptr, 2 * np.asarray(Xo.indices), Xo.data, Xo.n, 2 * Xo.d + 3)  # every odd column and the last ones empty
    y = np.random.default_rng(4).standard_normal(Xo.n)
    for reg in REGS:
        check_parity(X, y, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)
    check_parity(X, y, 3, "augment", True, True, "l21", maxIter=2, tol=0.0, gamma=1e-3)


@pytest.mark.parametrize("k", [1, 130])
def test_components(k):
    Xo, y = user_item(40, 50, 400, seed=7)
    for reg in REGS:
        check_parity(Xo, y, 2, "explicit", True, True, reg, k=k, maxIter=2, tol=0.0, gamma=1e-3)


def test_ml100k_shape():
    """943 users x 1682 items one-hot, 100 000 pairs, k = 4: the default regulariser (SquaredL21), 2 iterations"""
    Xo, y = user_item(943, 1682, 100000, seed=11)
    check_parity(Xo, y, 2, "explicit", True, True, "squaredl21", maxIter=2, tol=0.0, alpha0=1e-7, alpha=1e-5, beta=1e-3,
                 gamma=1e-4)


def test_callback_after_the_verbose_line(capsys):
    Xo, y = grid_data(2, "explicit", True, False)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    capsys.readouterr()
    nf.newPBCD(maxIter=1, tol=0.0).fit(csr_of(Xo), y, fm, callback=lambda o, f: print("callback"))
    lines = capsys.readouterr().out.splitlines()
    info = [i for i, line in enumerate(lines) if line.startswith("1 ")]
    assert len(info) == 1 and lines.count("callback") == 1, lines
    assert lines.index("callback") > info[0], lines
    # the verbose line's regularisation (pbcd.nim:303-306): the unscaled strengths
    opt = nf.newPBCD(maxIter=1, tol=0.0, verbose=0, reg=nf.newL21())
    want = 0.5 * opt.alpha0 * fm.intercept ** 2 + 0.5 * opt.alpha * (fm.w ** 2).sum() + 0.5 * opt.beta * (fm.P ** 2).sum() \
        + opt.gamma * np.sqrt((fm.P[0] ** 2).sum(0)).sum()
    np.testing.assert_allclose(opt._penalty(fm, 50.0) / 50.0, want, rtol=1e-12)


# ---------------------------------------------------------------- the schedule's edges (tests/cd_schedule_cases.py)
def device_schedule(Xo, reg):
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    fm.init(csr_of(Xo))
    return nf.newPBCD(verbose=0, reg=REGS[reg]()).schedule(csr_of(Xo), fm)


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_bit_equal(reg):
    """levels (L1, L21) and runs (SquaredL21) of 63, 64, 65, 1, 16, 17, 15, 130 and 5 features: k_pb_levels / k_pb_sq_runs three
    times per sweep, twice behind a wide launch; columns of 63, 64, 65, 1, 129 and 322 entries"""
    Xo, y = S.inputs("edges")
    assert device_schedule(Xo, reg) == (9, 130)
    for degree in degrees_of(reg)[:2]:
        for fit_linear in (True, False):
            check_parity(Xo, y, degree, "explicit", fit_linear, False, reg, exact=True, maxIter=3, tol=0.0,
                         gamma=S.gamma_of("edges", reg))


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_intercept_and_logistic(reg):
    Xo, y = S.inputs("edges")
    check_parity(Xo, y, 2 if reg == "squaredl21" else 3, "explicit", True, True, reg, task="classification", loss="logistic",
                 maxIter=3, tol=0.0, gamma=S.gamma_of("edges", reg))


@pytest.mark.parametrize("k", S.PBCD_K)
@pytest.mark.parametrize("reg", ["l21", "squaredl21"])
def test_schedule_edges_components(reg, k):
    """pb_grad's two layouts: k = 3 (4 lanes per sample, one idle), 5 (8 lanes), 32 (two samples in flight), 33 (one lane per
    component, a partial block), 64 (a full block), 65 (lanes_in_order continued across blocks)"""
    Xo, y = S.inputs("edges")
    check_parity(Xo, y, 2, "explicit", True, False, reg, k=k, exact=True, maxIter=3, tol=0.0, gamma=S.PBCD_K_GAMMA[reg][k])
    if reg == "l21" and k in (3, 33):
        check_parity(Xo, y, 3, "explicit", True, False, reg, k=k, exact=True, maxIter=2, tol=0.0, gamma=1e-3)


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_behind_empty_columns(reg):
    """beta = alpha = 0 with an unused id behind every feature: an empty column's invStepSize is clamped to 1e-12
    (pbcd.nim:148), so lam = gamma / 1e-12 and the prox takes the row to zero; everything stays finite"""
    Xo, y = S.inputs("edges_gaps")
    assert device_schedule(Xo, reg) == ((10, 130) if reg == "squaredl21" else (11, 331))
    empty = S.empty_columns("edges_gaps")
    fm, opt, _ = check_parity(Xo, y, 2, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, beta=0.0, alpha=0.0,
                              gamma=S.gamma_of("edges_gaps", reg))
    assert np.isfinite(fm.P).all() and np.isfinite(fm.w).all() and np.isfinite(np.array(opt.history)).all()
    assert np.all(fm.P[:, :, empty] == 0.0)
    check_parity(Xo, y, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, beta=0.0, alpha=0.0, gamma=S.gamma_of("edges_gaps", reg))


def test_schedule_long_sums_over_every_sample():
    """n = 2050: k_cd_intercept, k_pb_dummy and k_cd_loss take two full trips of their 1024 threads and a partial one"""
    Xo, y = S.inputs("long_1025")
    check_parity(Xo, y, 2, "explicit", True, True, "squaredl21", k=5, maxIter=2, tol=0.0, gamma=S.gamma_of("long_1025", "squaredl21"))
    check_parity(Xo, y, 3, "augment", True, True, "l21", k=5, maxIter=2, tol=0.0, gamma=S.gamma_of("long_1025", "l21"))


def test_schedule_long_wide_run_with_two_blocks_of_components():
    Xo, y = S.inputs("long_1025")
    assert device_schedule(Xo, "squaredl21") == (4, 1025)
    check_parity(Xo, y, 2, "explicit", True, False, "squaredl21", k=65, exact=True, maxIter=2, tol=0.0,
                 gamma=S.gamma_of("long_1025", "squaredl21"))


def test_direct_launches_equal_the_graph(tmp_path):
    compare_direct_launches("pbcd", "squaredl21", 2, tmp_path)


# ---------------------------------------------------------------- errors
def test_errors(tmp_path):
    L = capi.lib()
    Xo = random_csr(30, 10, 3, seed=1, sorted_idx=True)
    X = csr_of(Xo)
    y = np.ones(X.nSamples)
    with pytest.raises(ValueError, match="PBCD cannot be used for squaredl12."):
        nf.newPBCD(reg=nf.newSquaredL12())
    with pytest.raises(ValueError, match="transpose=true is not supported for BCD."):
        nf.newPBCD(reg=nf.newSquaredL21(transpose=True))
    with pytest.raises(ValueError):
        nf.newPBCD(reg=nf.newOmegaTI())
    with pytest.raises(ValueError, match="maxSearch"):
        nf.newPBCD(maxSearch=3)
    with pytest.raises(ValueError, match="shuffle"):
        nf.newPBCD(shuffle=True)
    nf.newPBCD(shrink=True)  # accepted and ignored
    with pytest.raises(ValueError, match="SquaredL21 supports only degree=2."):
        nf.newPBCD(verbose=0, maxIter=1).fit(X, y, nf.newFactorizationMachine("regression", degree=3, nComponents=3))
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3)
    fm.init(X)
    args = (1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0)
    for reg_id in (capi.REG["squaredl12"], capi.REG["omegati"]):
        h = _C.c_void_p()
        assert L.nfm_pbcd_create(fm._push(X.ctx), *args, reg_id, 0, _C.byref(h)) == capi.ERR_UNSUPPORTED
    h = _C.c_void_p()
    assert L.nfm_pbcd_create(fm._push(X.ctx), *args, capi.REG["squaredl12"], 0, _C.byref(h)) == capi.ERR_UNSUPPORTED
    assert b"PBCD cannot be used for squaredl12." in L.nfm_last_error()
    h = _C.c_void_p()
    assert L.nfm_pbcd_create(fm._push(X.ctx), *args, 7, 0, _C.byref(h)) == capi.ERR_INVALID
    h = _C.c_void_p()
    assert L.nfm_pbcd_create(fm._push(X.ctx), *args, capi.REG["l21"], 2, _C.byref(h)) == capi.ERR_UNSUPPORTED  # max_search
    fm3 = nf.newFactorizationMachine("regression", degree=3, nComponents=3)
    fm3.init(X)
    h = _C.c_void_p()
    assert L.nfm_pbcd_create(fm3._push(X.ctx), *args, capi.REG["squaredl21"], 0, _C.byref(h)) == capi.ERR_INVALID
    assert b"SquaredL21 supports only degree=2." in L.nfm_last_error()
    h = _C.c_void_p()
    assert L.nfm_pbcd_create(fm._push(X.ctx), *args, capi.REG["squaredl21"], 0, _C.byref(h)) == 0
    try:
        X.set_targets(y)
        assert L.nfm_cd_begin_fit(h, X.h) == 0
        assert L.nfm_opt_set_shuffle(h, 3) == capi.ERR_UNSUPPORTED
        assert L.nfm_opt_set_touch_cap(h, 4.0) == capi.ERR_UNSUPPORTED
        assert L.nfm_opt_set_ada_cross(h, 0.1) == capi.ERR_UNSUPPORTED
        ls, vs = _C.c_double(), _C.c_double()
        assert L.nfm_opt_epoch(h, X.h, None, 0, X.nSamples - 1, _C.byref(ls), _C.byref(vs)) == capi.ERR_INVALID
        assert L.nfm_opt_epoch(h, X.h, None, 0, X.nSamples, _C.byref(ls), _C.byref(vs)) == 0
    finally:
        L.nfm_opt_destroy(h)
    Xr = nf.newCSRDataset(np.ones(4), np.array([1, 1, 2, 3]), np.array([0, 2, 4]), 2, 5)  # a repeated id inside a row
    with pytest.raises(nf.NfmError) as e:
        nf.newPBCD(verbose=0, maxIter=1).fit(Xr, np.ones(2), nf.newFactorizationMachine("regression", degree=2, nComponents=2))
    assert e.value.code == capi.ERR_UNSUPPORTED
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)  # a field-aware model
    Xf = nf.newCSRFieldDataset(np.ones(4), np.array([0, 1, 2, 3]), np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2, 4, 2)
    ffm.init(Xf)
    hf = _C.c_void_p()
    assert L.nfm_pbcd_create(ffm._push(Xf.ctx), *args, 0, 0, _C.byref(hf)) == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        nf.newPBCD(verbose=0, maxIter=1).fit(Xf, np.ones(2), ffm)
    r = _cli(["train", "--task", "r", "--train", _files(tmp_path), "--solver", "pbcd"])  # the command line names the way
    assert r.returncode != 0 and "not supported" in r.stderr and "newPBCD" in r.stderr
