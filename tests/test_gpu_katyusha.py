"""-m gpu: Katyusha on the device (nfm_katyusha_create / nfm_katyusha_begin_fit / nfm_opt_epoch) against the plain-Python
restatement of the reference's loops (tests/katyusha_restatement.py) on the fixed inputs of tests/katyusha_cases.py: the
finalized model, every epoch's viol and lossVal, and the exact zero pattern of P.

Tolerance: MBPSGD's own bound (tests/test_gpu_psgd.py), rtol 1e-9 / atol 1e-12 on the parameters and 1e-10 relative on the
per-epoch scalars.  tests/test_katyusha_restatement.py bounds the restatement's own spread on these inputs by 1e-11."""
import ctypes as C
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
import katyusha_cases as Cs
from common import make_fm_dataset
from test_gpu_cd import csr_of

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
REGS = {"l1": lambda tr: nf.newL1(), "l21": lambda tr: nf.newL21(), "squaredl12": lambda tr: nf.newSquaredL12(True if tr is None else tr),
        "squaredl21": lambda tr: nf.newSquaredL21()}


def device_fit(name, verbose=0, callback=None, **over):
    c = Cs.case(name)
    skw = dict(c["skw"])
    Xo, y, P0, w0, b0, n_aug, stream = Cs.inputs(name)
    fm = nf.newFactorizationMachine(c["task"], degree=c["degree"], nComponents=P0.shape[1], fitLower=c["fit_lower"], fitLinear=c["fl"],
                                    fitIntercept=c["fi"], warmStart=True)
    fm.set_params(P0, w0, b0)
    reg = REGS[skw.pop("reg")](skw.pop("transpose", None))
    kw = dict(maxIter=c["max_iter"], tol=c["tol"], miniBatchSize=c["B"], verbose=verbose, reg=reg)
    kw.update(skw)
    kw.update(over)
    opt = nf.newKatyusha(**kw)
    X = csr_of(Xo)
    opt.fit(X, y, fm, callback=callback, stream=stream)
    return fm, opt, X


def check(name, fm, opt, r):
    assert len(opt.history) == len(r.iters), name
    for q, ((viol, lossVal), rs) in enumerate(zip(opt.history, r.iters)):
        print("%s epoch %d viol %.17g / %.17g lossVal %.17g / %.17g" % (name, q, viol, rs["viol"], lossVal, rs["lossVal"]))
        np.testing.assert_allclose(viol, rs["viol"], rtol=1e-10, atol=1e-300, err_msg="%s viol %d" % (name, q))
        np.testing.assert_allclose(lossVal, rs["lossVal"], rtol=1e-10, atol=1e-300, err_msg="%s lossVal %d" % (name, q))
    print("%s max |dP| %.3e of %.3e max |dw| %.3e |db| %.3e" % (name, np.abs(fm.P - r.P).max(), np.abs(r.P).max(), np.abs(fm.w - r.w).max(),
                                                                 abs(fm.intercept - r.b)))
    np.testing.assert_allclose(fm.P, r.P, rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_allclose(fm.w, r.w, rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_allclose(fm.intercept, r.b, rtol=RTOL, atol=ATOL, err_msg=name)
    assert np.array_equal(fm.P == 0.0, r.P == 0.0), name


@pytest.mark.parametrize("name", list(Cs.CASES) + list(Cs.GRID_CASES))
def test_parity_with_the_restatement(name):
    fm, opt, X = device_fit(name)
    s, r = Cs.restate(name)
    check(name, fm, opt, r)
    if name == "converges":
        assert r.converged and len(opt.history) < Cs.CASES[name]["max_iter"]
    if name == "wide_l1_k130":  # kc = 2 device blocks: L1 is fitted, a regulariser that couples a row's factors is still refused
        with pytest.raises(capi.NfmError):
            device_fit(name, reg=nf.newL21())
    if name == "flags_sqhinge_nolinear":  # the intercept only decays, and tilde's is 0 from the first epoch on (params.nim:47)
        assert r.tilde.b == 0.0 and fm.intercept != 0.05


@pytest.mark.parametrize("name", ["grid_sql12", "pad_l21_k17", "heavy", "deep_sql12_col"])
def test_two_runs_are_bitwise_equal(name):
    a, oa, _ = device_fit(name)
    b, ob, _ = device_fit(name)
    assert np.array_equal(a.P, b.P) and np.array_equal(a.w, b.w) and a.intercept == b.intercept
    assert oa.history == ob.history


def test_callback_sees_the_finalized_model_and_verbose_lines():
    name = "grid_l21"
    cb = []
    s, r = Cs.restate(name, verbose=1, callback=lambda P, w, b: cb.append((P, w, b)))
    seen = []
    out = io.StringIO()
    with redirect_stdout(out):
        fm, opt, _ = device_fit(name, verbose=1, callback=lambda o, m: seen.append((m.P.copy(), m.w.copy(), m.intercept, out.getvalue().count("\n"))))
    assert out.getvalue().splitlines() == r.lines
    assert len(seen) == len(cb) == len(r.iters)
    for q, ((P, w, b, lines_before), (Pr, wr, br)) in enumerate(zip(seen, cb)):
        np.testing.assert_allclose(P, Pr, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(w, wr, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(b, br, rtol=RTOL, atol=ATOL)
        assert lines_before == 3 + q  # the three header lines and q verbose lines: the callback comes before its epoch's line
    s, r = Cs.restate("converges", verbose=1)
    out = io.StringIO()
    with redirect_stdout(out):
        device_fit("converges", verbose=1)
    assert out.getvalue().splitlines() == r.lines and r.lines[-1].startswith("Converged at epoch")


def test_default_stream_and_identity_stream():
    """shuffle=False without a stream: indices[ii] with wrap-around, which is also what perm == NULL means to the C ABI"""
    name = "tau1_derived"
    c = Cs.CASES[name]
    Xo, y, P0, w0, b0, n_aug, _ = Cs.inputs(name)
    inner = (Xo.n - 1) // c["B"] + 1
    need = c["B"] * inner
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=P0.shape[1], warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = nf.newKatyusha(maxIter=1, tol=0.0, miniBatchSize=c["B"], verbose=0, reg=nf.newL1(), gamma=0.02, tau1=-1.0, shuffle=False)
    X = csr_of(Xo)
    opt.fit(X, y, fm)
    f2 = nf.newFactorizationMachine("regression", degree=2, nComponents=P0.shape[1], warmStart=True)
    f2.set_params(P0, w0, b0)
    o2 = nf.newKatyusha(maxIter=1, tol=0.0, miniBatchSize=c["B"], verbose=0, reg=nf.newL1(), gamma=0.02, tau1=-1.0)
    o2.fit(X, y, f2, stream=np.arange(need) % Xo.n)
    assert np.array_equal(fm.P, f2.P) and opt.history == o2.history
    # the same through perm == NULL
    L = capi.lib()
    f3 = nf.newFactorizationMachine("regression", degree=2, nComponents=P0.shape[1], warmStart=True)
    f3.set_params(P0, w0, b0)
    f3.init(X)
    X.set_targets(y)
    h = o2._handle(f3, X.ctx)  # at the mini-batch size of its fit
    assert L.nfm_katyusha_begin_fit(h, X.h) == 0
    ls, vs = C.c_double(0), C.c_double(0)
    assert L.nfm_opt_epoch(h, X.h, None, 0, need, C.byref(ls), C.byref(vs)) == 0
    f3._pull()
    assert np.array_equal(f3.P, f2.P) and (vs.value, ls.value / Xo.n) == o2.history[0]


def _create(L, mh, **kw):
    c = dict(eta=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, tau1=0.5, tau2=-1.0, loss=0, loss_param=1.0, reg=0, reg_transpose=0,
             batch=4)
    c.update(kw)
    h = C.c_void_p()
    rc = L.nfm_katyusha_create(mh, c["eta"], c["alpha0"], c["alpha"], c["beta"], c["gamma"], c["tau1"], c["tau2"], c["loss"], c["loss_param"],
                               c["reg"], c["reg_transpose"], c["batch"], C.byref(h))
    return rc, h


def test_refusals():
    L = capi.lib()
    Xo, _, y = make_fm_dataset(20, 6, 3, 4, 1)
    X = csr_of(Xo)

    def create(fm, **kw):
        fm.init(X)
        rc, h = _create(L, fm._push(X.ctx), **kw)
        if rc == 0:
            L.nfm_opt_destroy(h)
        return rc

    def message():
        return L.nfm_last_error().decode()

    fm3 = nf.newFactorizationMachine("regression", degree=3, nComponents=4)
    fm2 = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    nolin = nf.newFactorizationMachine("regression", degree=2, nComponents=4, fitLinear=False, fitIntercept=False)
    assert create(fm3, reg=capi.REG["squaredl12"], reg_transpose=1) == capi.ERR_INVALID and "SquaredL12 supports only degree=2." in message()
    assert create(fm3, reg=capi.REG["squaredl21"]) == capi.ERR_INVALID and "SquaredL21 supports only degree=2." in message()
    assert create(fm2, reg=capi.REG["omegati"]) == capi.ERR_UNSUPPORTED and "OmegaTI" in message()
    assert create(fm2, reg=capi.REG["squaredl21"], reg_transpose=1) == capi.ERR_UNSUPPORTED and "transpose" in message()
    assert create(fm2, beta=0.0) == capi.ERR_INVALID and "beta must be > 0" in message()
    assert create(fm2, alpha=0.0) == capi.ERR_INVALID and "alpha must be > 0 with fitLinear" in message()
    assert create(fm2, alpha0=0.0) == capi.ERR_INVALID and "alpha0 must be > 0 with fitIntercept" in message()
    assert create(nolin, alpha=0.0, alpha0=0.0) == 0  # neither strength is read
    assert create(fm2, eta=0.0) == capi.ERR_INVALID and "eta must be > 0" in message()
    assert create(fm2, batch=0) == capi.ERR_INVALID and create(fm2, batch=2 ** 31) == capi.ERR_INVALID and "miniBatchSize" in message()
    assert create(fm2) == 0
    wide = nf.newFactorizationMachine("regression", degree=2, nComponents=130)
    assert create(wide, reg=capi.REG["l21"]) == capi.ERR_UNSUPPORTED and "n_components > 128" in message()
    assert create(wide, reg=capi.REG["l1"]) == 0
    # the hosts: ValueError
    with pytest.raises(ValueError, match="reg must be one of"):
        nf.newKatyusha(reg=nf.newOmegaTI())
    with pytest.raises(ValueError, match="once per epoch"):
        nf.newKatyusha(nCalls=3)
    with pytest.raises(ValueError, match="beta must be > 0"):
        nf.newKatyusha(beta=0.0)
    with pytest.raises(ValueError, match="eta must be > 0"):
        nf.newKatyusha(eta=-1.0)
    with pytest.raises(ValueError, match="alpha must be > 0 with fitLinear"):
        nf.newKatyusha(alpha=0.0, verbose=0).fit(X, y, nf.newFactorizationMachine("regression", nComponents=2))
    with pytest.raises(ValueError, match="alpha0 must be > 0 with fitIntercept"):
        nf.newKatyusha(alpha0=0.0, verbose=0).fit(X, y, nf.newFactorizationMachine("regression", nComponents=2))
    with pytest.raises(ValueError, match="supports only degree=2"):
        nf.newKatyusha(verbose=0).fit(X, y, nf.newFactorizationMachine("regression", degree=3, nComponents=2))
    # a field-aware model: ValueError from the Python host, NFM_ERR_UNSUPPORTED from the C ABI itself
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)
    with pytest.raises(ValueError):
        nf.newKatyusha(verbose=0).fit(X, y, ffm)
    n, d, F = 8, 6, 3
    rng = np.random.default_rng(0)
    idx = np.stack([np.sort(rng.choice(d, 3, replace=False)) for _ in range(n)]).astype(np.int64)
    Xf = nf.newCSRFieldDataset(rng.uniform(-1, 1, n * 3), idx.ravel(), np.arange(n + 1, dtype=np.int64) * 3, (idx % F).ravel(), n, d, F)
    ffm.init(Xf)
    rc, _ = _create(L, ffm._push(Xf.ctx))
    assert rc == capi.ERR_UNSUPPORTED and "FactorizationMachine" in message()
    # the epoch call's rules
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    opt = nf.newKatyusha(maxIter=1, verbose=0, reg=nf.newL1(), miniBatchSize=8)
    opt.fit(X, y, fm)
    ls, vs = C.c_double(0), C.c_double(0)
    n = X.nSamples  # 20: three mini-batches of 8
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID and "outer iteration" in message()
    bad = np.full(24, n, dtype=np.int64)
    assert L.nfm_opt_epoch(opt._h, X.h, bad.ctypes.data_as(C.c_void_p), 0, 24, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, 24, C.byref(ls), C.byref(vs)) == 0
    assert L.nfm_opt_finalize(opt._h) == 0
    assert L.nfm_opt_set_shuffle(opt._h, 1) == capi.ERR_UNSUPPORTED
    assert L.nfm_opt_set_touch_cap(opt._h, 2.0) == capi.ERR_UNSUPPORTED
    ctxs = (C.c_void_p * 1)(X.ctx.h.value)
    grp = (C.c_void_p * 1)()
    assert L.nfm_dp_create_local(ctxs, 1, grp) == 0
    try:
        assert L.nfm_opt_set_dp(opt._h, grp[0], 0, 0) == capi.ERR_UNSUPPORTED
    finally:
        L.nfm_dp_destroy(grp[0])
    # no begin_fit on this dataset: another dataset, the same dataset after its targets changed, a fresh handle
    X2 = csr_of(Xo)
    X2.set_targets(y)
    assert L.nfm_opt_epoch(opt._h, X2.h, None, 0, 24, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID and "nfm_katyusha_begin_fit" in message()
    X.set_targets(y + 1.0)
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, 24, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    fresh = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    fresh.init(X)
    rc, h = _create(L, fresh._push(X.ctx))
    assert rc == 0
    assert L.nfm_opt_epoch(h, X.h, None, 0, 20, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    L.nfm_opt_destroy(h)
    # a repeated column id in a row
    Xr = nf.newCSRDataset(np.ones(4), np.array([0, 0, 1, 2]), np.array([0, 2, 4]), 2, 6)
    with pytest.raises(capi.NfmError) as ei:
        nf.newKatyusha(maxIter=1, verbose=0, reg=nf.newL1()).fit(Xr, np.zeros(2), nf.newFactorizationMachine("regression", nComponents=2))
    assert ei.value.code == capi.ERR_UNSUPPORTED
