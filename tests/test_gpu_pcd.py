"""-m gpu: proximal coordinate descent (newPCD, optimizer/pcd.nim) on the device -- nfm_pcd_create / nfm_cd_begin_fit /
nfm_opt_epoch -- against the plain-Python restatement of the reference's loop (tests/pcd_restatement.py).

L1 and row-wise SquaredL12 run CD's level schedule; column-wise SquaredL12 (the default) and OmegaTI the run schedule.
Tolerances as CD's: with squared loss, no intercept and no dummy features P, w and viol are BIT-equal to the restatement in
the reference's order; the intercept's, the dummy features' and the loss's sums over all samples are a fixed tree on the
device: 1e-10 relative there."""
import ctypes as _C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
from common import init_fm, make_fm_dataset, random_csr
import cd_schedule_cases as S
import pcd_restatement as R
from cd_direct_child import compare as compare_direct_launches
from test_gpu_cd import Csr, csr_of, user_item

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
N, D, K = 50, 6, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGS = {"l1": lambda: nf.newL1(), "sq_row": lambda: nf.newSquaredL12(transpose=False), "sq_col": lambda: nf.newSquaredL12(),
        "ti": lambda: nf.newOmegaTI()}
RESTATED = {"l1": ("l1", False), "sq_row": ("squaredl12", False), "sq_col": ("squaredl12", True), "ti": ("omegati", False)}


def degrees_of(reg):
    return (2,) if reg.startswith("sq") else (2, 3, 4)


def device_fit(X, y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, reg, task="regression", **kw):
    fm = nf.newFactorizationMachine(task, degree=degree, nComponents=P0.shape[1], fitLower=fit_lower, fitLinear=fit_linear,
                                    fitIntercept=fit_intercept, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = nf.newPCD(verbose=0, reg=REGS[reg](), **kw)
    opt.fit(X, y, fm)
    return fm, opt


def check_parity(Xo, y, degree, fit_lower, fit_linear, fit_intercept, reg, k=K, task="regression", seed=1, exact=False,
                 **kw):
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fit_linear, seed=seed, scale=0.1)
    w0 = np.random.default_rng(seed + 5).uniform(-0.1, 0.1, Xo.d) if fit_linear else w0
    b0 = 0.05 if fit_intercept else 0.0
    fm, opt = device_fit(csr_of(Xo), y, P0, w0, b0, degree, fit_lower, fit_linear, fit_intercept, reg, task=task, **kw)
    name, tr = RESTATED[reg]
    P, w, b, hist, _ = R.fit(Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept,
                             task=task, reg=name, transpose=tr, **kw)
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
# (tests/test_pcd_l1.nim, test_pcd_squaredl12.nim, test_pcd_ti.nim)
@pytest.mark.parametrize("reg,degree,fit_lower", SUITE)
def test_reference_suite(reg, degree, fit_lower):
    for fit_intercept in (True, False):  # fitLinear = false leaves w at 0
        Xo, y = grid_data(degree, fit_lower, False, fit_intercept, threshold=0.0)
        fm = new_fm(degree, fit_lower, False, fit_intercept)
        nf.newPCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(csr_of(Xo), y, fm)
        assert np.all(fm.w == 0.0)
    for fit_linear in (True, False):  # fitIntercept = false leaves the intercept at 0
        Xo, y = grid_data(degree, fit_lower, fit_linear, False, threshold=0.0)
        fm = new_fm(degree, fit_lower, fit_linear, False)
        nf.newPCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(csr_of(Xo), y, fm)
        assert fm.intercept == 0.0
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):
        Xo, y = grid_data(degree, fit_lower, fit_linear, fit_intercept, threshold=0.0)
        X = csr_of(Xo)
        warm = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)  # warm start
        opt = nf.newPCD(maxIter=1, verbose=0, tol=0, reg=REGS[reg]())
        for _ in range(10):
            opt.fit(X, y, warm)
        cold = new_fm(degree, fit_lower, fit_linear, fit_intercept)
        nf.newPCD(maxIter=10, verbose=0, tol=0, reg=REGS[reg]()).fit(X, y, cold)
        assert abs(cold.intercept - warm.intercept) < 1e-8
        np.testing.assert_allclose(cold.w, warm.w, atol=1e-8, rtol=0)
        np.testing.assert_allclose(cold.P, warm.P, atol=1e-8, rtol=0)
        fm = new_fm(degree, fit_lower, fit_linear, fit_intercept)  # the score decreases
        fm.init(X)
        before = fm.score(X, y)
        nf.newPCD(maxIter=20, verbose=0, tol=0, alpha0=1e-9, alpha=1e-9, beta=1e-9, gamma=1e-9, reg=REGS[reg]()).fit(X, y, fm)
        assert fm.score(X, y) < before
    for fit_linear, fit_intercept in itertools.product((True, False), (True, False)):  # strong vs weak regularisation
        Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept, scale=1.0)
        X = csr_of(Xo)
        weak = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        strong = new_fm(degree, fit_lower, fit_linear, fit_intercept, warmStart=True)
        nf.newPCD(maxIter=100, verbose=0, tol=0, alpha0=0, alpha=0, beta=0, gamma=0, reg=REGS[reg]()).fit(X, y, weak)
        nf.newPCD(maxIter=100, verbose=0, tol=0, alpha0=1e5, alpha=1e5, beta=1e5, gamma=1e5, reg=REGS[reg]()).fit(X, y, strong)
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
    if not reg.startswith("sq"):
        Xo, y = grid_data(3, "explicit", True, True)
        check_parity(Xo, y, 3, "explicit", True, True, reg, task=task, maxIter=3, tol=0.0, gamma=1e-3, loss=loss)


@pytest.mark.parametrize("reg", list(REGS))
def test_bit_equal_to_the_reference_order(reg):
    for degree in degrees_of(reg):
        for name, (Xo, y) in {"grid": grid_data(degree, "explicit", True, False),
                              "user_item": user_item(30, 40, 300, seed=3)}.items():
            for fit_linear in (True, False):
                check_parity(Xo, y, degree, "explicit", fit_linear, False, reg, exact=True, maxIter=4, tol=0.0, gamma=1e-3)


# ---------------------------------------------------------------- the schedules
def _example_012():
    return Csr([0, 2, 3, 4], [0, 1, 1, 2], [1.0, 0.5, -0.7, 1.3], 3, 3), np.array([1.0, -0.5, 2.0])


def test_chain_example_and_user_item_runs():
    Xo, y = _example_012()
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=2, fitLinear=False, fitIntercept=False)
    fm.init(csr_of(Xo))
    assert nf.newPCD(verbose=0).schedule(csr_of(Xo), fm) == (2, 2)  # runs [0], [1, 2]
    fm2, _, P = check_parity(Xo, y, 2, "explicit", False, False, "sq_col", k=2, exact=True, maxIter=3, tol=0.0, beta=1e-3,
                             gamma=0.05)
    assert (P == 0.0).any()
    Xu, yu = user_item(60, 80, 900, seed=5)
    fmu = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
    fmu.init(csr_of(Xu))
    assert nf.newPCD(verbose=0).schedule(csr_of(Xu), fmu) == (2, 80)  # the users, then the items
    assert nf.newPCD(verbose=0, reg=nf.newL1()).schedule(csr_of(Xu), fmu)[0] == 2  # levels
    check_parity(Xu, yu, 2, "explicit", True, False, "sq_col", exact=True, maxIter=3, tol=0.0, gamma=1e-3)
    check_parity(Xu, yu, 2, "explicit", True, True, "ti", maxIter=3, tol=0.0, gamma=1e-3)


def test_wide_levels_and_wide_runs():
    """user x item with 80 items: the item level (run) is >= 64 features, a launch of its own -- k_cd_level for the local
    regularisers, k_pcd_grad / k_pcd_chain / k_pcd_sync for the chained ones, at degree 2 and 3"""
    Xu, yu = user_item(60, 80, 900, seed=5)
    for reg in ("l1", "sq_row"):
        check_parity(Xu, yu, 2, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, gamma=1e-3)
        check_parity(Xu, yu, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)
    for reg in ("l1", "ti"):
        check_parity(Xu, yu, 3, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, gamma=1e-3)
        check_parity(Xu, yu, 3, "augment", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)


def test_l1_zero_pattern():
    Xo, y = grid_data(2, "explicit", True, False)
    _, _, P = check_parity(Xo, y, 2, "explicit", True, False, "l1", exact=True, maxIter=5, tol=0.0, gamma=0.05)
    assert 0 < (P == 0.0).sum() < P.size


def test_empty_columns_and_unsorted_rows():
    Xo = random_csr(120, 60, 5, seed=8, sorted_idx=False)
    X = Csr(Xo.indptr, 2 * np.asarray(Xo.indices), Xo.data, Xo.n, 2 * Xo.d + 3)  # every odd column and the last ones empty
    y = np.random.default_rng(4).standard_normal(Xo.n)
    for reg in REGS:
        check_parity(X, y, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, gamma=1e-3)
    check_parity(X, y, 3, "augment", True, True, "ti", maxIter=2, tol=0.0, gamma=1e-3)


@pytest.mark.parametrize("k", [1, 130])
def test_components(k):
    Xo, y = user_item(40, 50, 400, seed=7)
    for reg in REGS:
        check_parity(Xo, y, 2, "explicit", True, True, reg, k=k, maxIter=2, tol=0.0, gamma=1e-3)


def test_ml100k_shape():
    """943 users x 1682 items one-hot, 100 000 pairs, k = 4: the default regulariser (column-wise SquaredL12), 2 iterations"""
    Xo, y = user_item(943, 1682, 100000, seed=11)
    check_parity(Xo, y, 2, "explicit", True, True, "sq_col", maxIter=2, tol=0.0, alpha0=1e-7, alpha=1e-5, beta=1e-3,
                 gamma=1e-4)


def test_callback_and_verbose_order(capsys):
    """the fit loop CD and PCD share: CD's callback runs before the iteration's verbose line (cd.nim), PCD's after it
    (pcd.nim:188-192)"""
    Xo, y = grid_data(2, "explicit", True, False)
    for opt, first in ((nf.newCD(maxIter=1, tol=0.0), True), (nf.newPCD(maxIter=1, tol=0.0), False)):
        fm = nf.newFactorizationMachine("regression", degree=2, nComponents=K)
        capsys.readouterr()
        opt.fit(csr_of(Xo), y, fm, callback=lambda o, f: print("callback"))
        lines = capsys.readouterr().out.splitlines()
        info = [i for i, line in enumerate(lines) if line.startswith("1 ")]
        assert len(info) == 1 and lines.count("callback") == 1, lines
        assert (lines.index("callback") < info[0]) == first, lines


# ---------------------------------------------------------------- the schedule's edges (tests/cd_schedule_cases.py)
def device_schedule(Xo, reg, degree=2):
    fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=K)
    fm.init(csr_of(Xo))
    return nf.newPCD(verbose=0, reg=REGS[reg]()).schedule(csr_of(Xo), fm)


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_bit_equal(reg):
    """levels (L1, row-wise SquaredL12) and runs (column-wise SquaredL12, OmegaTI) of 63, 64, 65, 1, 16, 17, 15, 130 and 5
    features: the one-workgroup walk three times per sweep, twice behind a wide launch, the chain handed narrow -> wide -> wide
    -> narrow -> wide -> narrow; columns of 63, 64, 65, 1, 129 and 322 entries"""
    Xo, y = S.inputs("edges")
    assert device_schedule(Xo, reg) == R.schedule(Xo.indptr, Xo.indices, Xo.n, Xo.d, reg in ("sq_col", "ti")) == (9, 130)
    for degree in degrees_of(reg):
        for fit_linear in (True, False):
            check_parity(Xo, y, degree, "explicit", fit_linear, False, reg, exact=True, maxIter=3, tol=0.0,
                         gamma=S.gamma_of("edges", reg))


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_intercept_and_logistic(reg):
    Xo, y = S.inputs("edges")
    check_parity(Xo, y, 2 if reg.startswith("sq") else 3, "explicit", True, True, reg, task="classification", loss="logistic",
                 maxIter=3, tol=0.0, gamma=S.gamma_of("edges", reg))


@pytest.mark.parametrize("reg", list(REGS))
def test_schedule_edges_behind_empty_columns(reg):
    """beta = alpha = 0 with an unused id behind every feature: every empty column is a skipped step (invStepSize < 1e-12,
    pcd.nim:57,100) inside a narrow run (k_pcd_runs) or a wide one (k_pcd_chain leaves sn[f] unwritten, k_pcd_sync returns), or
    in the wide level 0 (k_cd_level): P stays as it started there, bit for bit, and the chain does not move"""
    Xo, y = S.inputs("edges_gaps")
    chained = reg in ("sq_col", "ti")
    assert device_schedule(Xo, reg) == R.schedule(Xo.indptr, Xo.indices, Xo.n, Xo.d, chained) == ((10, 130) if chained else (11, 331))
    empty = S.empty_columns("edges_gaps")
    for degree in degrees_of(reg)[:2]:
        fm, opt, _ = check_parity(Xo, y, degree, "explicit", True, False, reg, exact=True, maxIter=3, tol=0.0, beta=0.0,
                                  alpha=0.0, gamma=S.gamma_of("edges_gaps", reg))
        P0, w0, _, _ = S.start(Xo, degree, K, "explicit", True, False)
        assert np.array_equal(fm.P[:, :, empty], P0[:, :, empty]) and np.array_equal(fm.w[empty], w0[empty])
        assert np.isfinite(fm.P).all() and np.isfinite(fm.w).all() and np.isfinite(np.array(opt.history)).all()
    check_parity(Xo, y, 2, "explicit", True, True, reg, maxIter=3, tol=0.0, beta=0.0, alpha=0.0, gamma=S.gamma_of("edges_gaps", reg))


@pytest.mark.parametrize("reg", ["l1", "ti"])
def test_schedule_long_sums_over_every_sample(reg):
    """n = 2050: k_cd_intercept, k_cd_dummy (the chain continued into the dummy feature) and k_cd_loss take two full trips of
    their 1024 threads and a partial one; the first run is 1025 features wide"""
    Xo, y = S.inputs("long_1025")
    check_parity(Xo, y, 3, "augment", True, True, reg, task="classification", loss="logistic", maxIter=2, tol=0.0,
                 gamma=S.gamma_of("long_1025", reg))


@pytest.mark.parametrize("name", ["long_1024", "long_1025"])
def test_schedule_long_chain_chunks(name):
    """k_pcd_chain stages kNarrowBlock = 1024 features at a time: a run of exactly one chunk, and one of a chunk and a feature"""
    Xo, y = S.inputs(name)
    assert device_schedule(Xo, "sq_col") == (4, int(name[-4:]))
    check_parity(Xo, y, 2, "explicit", True, False, "sq_col", exact=True, maxIter=2, tol=0.0, gamma=S.gamma_of(name, "sq_col"))


def test_direct_launches_equal_the_graph(tmp_path):
    compare_direct_launches("pcd", "sq_col", 2, tmp_path)


# ---------------------------------------------------------------- errors
def test_errors():
    L = capi.lib()
    Xo = random_csr(30, 10, 3, seed=1, sorted_idx=True)
    X = csr_of(Xo)
    y = np.ones(X.nSamples)
    for reg, msg in ((nf.newL21(), "PCD cannot be used for L21."), (nf.newSquaredL21(), "PCD cannot be used for squaredL21.")):
        with pytest.raises(ValueError, match=msg):
            nf.newPCD(reg=reg)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3)
    fm.init(X)
    for reg_id in (capi.REG["l21"], capi.REG["squaredl21"]):
        h = _C.c_void_p()
        assert L.nfm_pcd_create(fm._push(X.ctx), 1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0, reg_id, 0, _C.byref(h)) == capi.ERR_UNSUPPORTED
    h = _C.c_void_p()
    assert L.nfm_pcd_create(fm._push(X.ctx), 1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0, 7, 0, _C.byref(h)) == capi.ERR_INVALID
    fm3 = nf.newFactorizationMachine("regression", degree=3, nComponents=3)
    fm3.init(X)
    h = _C.c_void_p()
    assert L.nfm_pcd_create(fm3._push(X.ctx), 1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0, capi.REG["squaredl12"], 1, _C.byref(h)) == \
        capi.ERR_INVALID
    with pytest.raises(ValueError, match="SquaredL12 supports only degree=2."):
        nf.newPCD(verbose=0, maxIter=1).fit(X, y, nf.newFactorizationMachine("regression", degree=3, nComponents=3))
    h = _C.c_void_p()
    assert L.nfm_pcd_create(fm._push(X.ctx), 1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0, capi.REG["omegati"], 0, _C.byref(h)) == 0
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
        nf.newPCD(verbose=0, maxIter=1).fit(Xr, np.ones(2), nf.newFactorizationMachine("regression", degree=2, nComponents=2))
    assert e.value.code == capi.ERR_UNSUPPORTED
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)  # a field-aware model
    Xf = nf.newCSRFieldDataset(np.ones(4), np.array([0, 1, 2, 3]), np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2, 4, 2)
    ffm.init(Xf)
    hf = _C.c_void_p()
    assert L.nfm_pcd_create(ffm._push(Xf.ctx), 1e-6, 1e-3, 1e-4, 1e-4, 0, 1.0, 0, 0, _C.byref(hf)) == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):  # OmegaTI has no matrix prox: MBPSGD refuses it in the host
        nf.newMBPSGD(reg=nf.newOmegaTI())


# ---------------------------------------------------------------- the command line
def _files(tmp_path):
    rng = np.random.default_rng(3)
    lines = []
    for _ in range(60):
        cols = sorted(rng.choice(12, 3, replace=False))
        lines.append("%.3f " % rng.standard_normal() + " ".join("%d:%.3f" % (c, rng.uniform(0.1, 1)) for c in cols))
    p = tmp_path / "train.svm"
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def _cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "nimfm_amd"] + args, capture_output=True, text=True, env=env, timeout=600)


def test_cli(tmp_path):
    train = _files(tmp_path)
    dump = str(tmp_path / "fm.txt")
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "pcd", "--reg", "l1", "--gamma", "1e-3", "--maxIter", "5",
              "--nComponents", "3", "--verbose", "0", "--dump", dump])
    assert r.returncode == 0, r.stderr
    fm = nf.load(dump, False)
    assert fm.P.shape[1] == 3 and np.isfinite(fm.P).all()
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "pcd", "--maxIter", "2", "--verbose", "1"])
    assert r.returncode == 0, r.stderr
    for reg, msg in (("l21", "PCD cannot be used for L21."), ("squaredl21", "PCD cannot be used for squaredL21.")):
        r = _cli(["train", "--task", "r", "--train", train, "--solver", "pcd", "--reg", reg])
        assert r.returncode != 0 and msg in r.stderr
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "pbcd"])
    assert r.returncode != 0 and "not supported" in r.stderr
