"""CPU: what makes the device comparisons of tests/test_gpu_psgd_lazy.py meaningful.  The restatement of optimizer/psgd.nim
with the lazy hooks of L1 and L21 (tests/psgd_lazy_restatement.py) is held to the reference's own checks -- the dense solver
at gamma = 0 and the warm start (tests/test_psgd_l1.nim:63-135) -- and the cases the device runs (tests/psgd_lazy_cases.py) are
held to the properties the device tests rely on."""
import warnings

import numpy as np
import pytest

import common
import psgd_lazy_cases as CS
import psgd_lazy_restatement as R


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("grid", CS.GRID, ids=lambda g: "deg%d-%s-lin%d-int%d" % g)
def test_lazy_equals_dense_at_gamma_zero(grid, reg):
    """test_psgd_l1.nim:99-135, within its bounds: checkAlmostEqual's defaults (rtol 1e-6, atol 1e-9) and 1e-7 on the intercept.
    At gamma = 0 only, as the reference compares: the lazy L1 threshold uses the scaling BEFORE the step, so it is not the
    composition of the dense per-step thresholds."""
    case = CS.grid_case(*grid, gamma=0.0)
    lazy = case.restate(reg)
    kw = dict(case.model)
    kw.update(case.solver)
    kw.pop("tol")
    dense = R.psgd_slow_fit(case.X.dense(), case.y, case.P0, case.w0, case.b0, reg=reg, perms=case.perms, **kw)
    assert abs(lazy.intercept - dense.intercept) < 1e-7
    common.assert_close(lazy.w, dense.w, what="w")
    common.assert_close(lazy.P, dense.P, what="P")
    if not case.model["fit_linear"]:
        assert not lazy.w.any()
    if not case.model["fit_intercept"]:
        assert lazy.intercept == 0.0


@pytest.mark.parametrize("reg", CS.REGS)
def test_warm_start(reg):
    """test_psgd_l1.nim:63-96: ten fits of one epoch equal one fit of ten epochs with shuffle = false, atol 1e-8"""
    for grid in ((2, "explicit", True, True), (3, "augment", True, False), (4, "none", False, True)):
        case = CS.grid_case(*grid)
        once = case.restate(reg, maxIter=10, perms=None)
        P, w, b, it = case.P0, case.w0, case.b0, 1
        X = case.X
        kw = dict(case.model)
        kw.update(case.solver)
        kw.update(maxIter=1, reg=reg)
        for _ in range(10):
            r = R.psgd_fit(X.indptr, X.indices, X.data, X.n, X.d, case.y, P, w, b, it=it, **kw)
            P, w, b, it = r.P, r.w, r.intercept, r.it
        assert it == once.it == 801
        assert abs(b - once.intercept) < 1e-8
        common.assert_close(w, once.w, atol=1e-8, what="w")
        common.assert_close(P, once.P, atol=1e-8, what="P")


def test_every_device_case_keeps_its_thresholds_clear():
    """the smallest relative distance between a thresholded magnitude and its threshold is at least 1e-6 in every case the device
    runs: a device result within rtol 1e-9 cannot land on the other side of any threshold, so the zero patterns are compared
    with no entry exempt"""
    worst = {}
    for case, reg in CS.device_cases():
        ref = case.reference(reg)
        assert ref.record.thresholds_taken > 0
        assert np.isfinite(ref.P).all() and np.isfinite(ref.w).all(), (case.name, reg)
        assert len(ref.losses) == case.epochs and np.isfinite(ref.losses).all(), (case.name, reg)
        worst[(case.name, reg)] = ref.record.min_margin
    name = min(worst, key=worst.get)
    print("smallest margin %.3e at %s" % (worst[name], name))
    assert worst[name] >= 1e-6, (name, worst[name])


def test_sparse_cases_are_partly_zero():
    for case, reg in CS.sparse_cases():
        share = float((case.reference(reg).P == 0.0).mean())
        print("%s: %.0f %% zeros" % (case.name, 100 * share))
        assert 0.2 <= share <= 0.8, (case.name, share)


@pytest.mark.parametrize("reg", CS.REGS)
def test_reset_cases_reset(reg):
    cr = CS.cache_reset_case().reference(reg)
    assert cr.record.cache_resets >= 1 and np.isfinite(cr.P).all() and cr.P.any()
    wr = CS.w_reset_case().reference(reg)
    assert wr.record.w_resets >= 1 and np.isfinite(wr.w).all()
    print("%s: %d cache resets, %d w resets" % (reg, cr.record.cache_resets, wr.record.w_resets))


def test_l1_reset_consistent_is_a_catch_up_and_the_reference_lines_are_not():
    """L1's cache reset: lazyUpdateFinal's formula (what the device does) agrees with a fit that never resets to 1e-12 of max|P|;
    the reference's lines (l1.nim:113-126) do not -- the result is non-finite or differs by more than 1e-3 of max|P|"""
    case = CS.cache_reset_case()
    never = case.restate("l1", resets=False)
    consistent = case.reference("l1")
    assert consistent.record.cache_resets >= 1 and never.record.cache_resets == 0
    scale = np.abs(never.P).max()
    assert scale > 0
    assert np.abs(consistent.P - never.P).max() <= 1e-12 * scale
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (overflow is the point)
        as_written = case.restate("l1", l1_reset="reference")
    assert as_written.record.cache_resets >= 1
    assert not np.isfinite(as_written.P).all() or np.abs(as_written.P - never.P).max() > 1e-3 * scale
