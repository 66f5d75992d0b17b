"""-m gpu: PGD, FISTA and NMAPGD on the device (nfm_pgd_create / nfm_pgd_begin_fit / nfm_opt_epoch / nfm_pgd_last_iter)
against the plain-Python restatement of the reference's loops (tests/pgd_restatement.py) on the fixed inputs of
tests/pgd_cases.py.

Every iteration's trial counts and branches equal the restatement's exactly, and so does the final step size of PGD and
FISTA.  NMAPGD's line search starts at the Barzilai-Borwein ratio of two sums, which the device adds with a fixed tree and
nfm_pgd_last_iter reports: that START is compared at 1e-10 relative, and the final step size must be EXACTLY the device's
start multiplied by rho as many times as the restatement shrank its own (eta / start is the restatement's rho^m, bit for
bit).  P, w, the intercept,
lossVal, regVal and viol: 1e-10 relative where only fixed-tree sums differ (L1, L21, row-wise SquaredL12), 1e-9 with the
exact zero pattern where the deterministic threshold iteration stands in for the reference's pivoting (column-wise
SquaredL12, SquaredL21).  The restatement's own spread between summation orders is at most 3.3e-12 on these inputs
(tests/test_pgd_restatement.py), below a tenth of either tolerance, so neither is widened."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
import dense_grid_cases as G
import pgd_cases as Cs
import pgd_restatement as R
from common import init_fm, make_fm_dataset, random_csr
from test_gpu_cd import csr_of

pytestmark = pytest.mark.gpu
REGS = {"l1": lambda tr: nf.newL1(), "l21": lambda tr: nf.newL21(), "squaredl12": lambda tr: nf.newSquaredL12(True if tr is None else tr),
        "squaredl21": lambda tr: nf.newSquaredL21()}
RHO = 0.5  # every fixed input keeps the default rho
NEW = {"pgd": nf.newPGD, "fista": nf.newFISTA, "nmapgd": nf.newNMAPGD}


def tol_of(skw):
    coupled = (skw["reg"] == "squaredl12" and skw.get("transpose", True)) or skw["reg"] == "squaredl21"
    return (1e-9, True) if coupled else (1e-10, False)


def device_opt(algo, skw, fkw, verbose=0):
    kw = {k: v for k, v in skw.items() if k not in ("reg", "transpose", "task", "max_search", "loss_param")}
    if "max_search" in skw:
        kw["maxSearch"] = skw["max_search"]
    return NEW[algo](maxIter=fkw["max_iter"], tol=fkw["tol"], verbose=verbose, reg=REGS[skw["reg"]](skw.get("transpose")), **kw)


def device_fit(name, verbose=0, callback=None, **fit_over):
    algo, degree, fit_lower, fl, fi, skw, fkw = Cs.CASES[name]
    fkw = dict(fkw, **fit_over)
    Xo, y, P0, w0, b0, n_aug = Cs.inputs(name)
    fm = nf.newFactorizationMachine(skw.get("task", "regression"), degree=degree, nComponents=P0.shape[1], fitLower=fit_lower,
                                    fitLinear=fl, fitIntercept=fi, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = device_opt(algo, skw, fkw, verbose)
    X = csr_of(Xo)
    opt.fit(X, y, fm, callback=callback)
    return fm, opt, X, Xo


def check_iterations(name, opt, r, rtol, algo=None):
    algo = Cs.CASES[name][0] if algo is None else algo
    assert len(opt.iterations) == len(r.iters), name
    for q, (dv, rs) in enumerate(zip(opt.iterations, r.iters)):
        tag = "%s iteration %d" % (name, q)
        assert dv["trials"] == tuple(rs["trials"]), tag
        assert dv["branch"] == rs["branch"], tag
        for which in (0, 1):
            if rs["trials"][which] == 0:
                assert dv["eta"][which] == 0.0 and dv["start"][which] == 0.0, tag
                continue
            m, e = 0, rs["start"][which]  # how often the restatement multiplied by rho
            while e != rs["eta"][which]:
                e *= RHO
                m += 1
                assert m <= 64, tag
            if algo == "nmapgd":  # the start is a ratio of two fixed-tree sums
                np.testing.assert_allclose(dv["start"][which], rs["start"][which], rtol=1e-10, atol=0, err_msg=tag)
            else:
                assert dv["start"][which] == rs["start"][which] == 1.0, tag
            e = dv["start"][which]
            for _ in range(m):
                e *= RHO
            assert dv["eta"][which] == e, tag  # exactly start * rho^m, m the restatement's
            if algo != "nmapgd":
                assert dv["eta"][which] == rs["eta"][which], tag
        for key in ("lossVal", "regVal", "viol", "t", "c", "q"):
            print("%s %s device %.17g restatement %.17g" % (tag, key, dv[key], rs[key]))
            np.testing.assert_allclose(dv[key], rs[key], rtol=rtol, atol=1e-300, err_msg=tag + " " + key)


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_parity_with_the_restatement(name):
    skw = Cs.CASES[name][5]
    rtol, zeros = tol_of(skw)
    fm, opt, X, Xo = device_fit(name)
    s, r = Cs.restate(name)
    check_iterations(name, opt, r, rtol)
    atol = rtol * max(np.abs(r.P).max(), 1e-300) * 1e-2
    print("%s max |dP| %.3e max |dw| %.3e |db| %.3e" % (name, np.abs(fm.P - r.P).max(), np.abs(fm.w - r.w).max(), abs(fm.intercept - r.b)))
    np.testing.assert_allclose(fm.P, r.P, rtol=rtol, atol=atol, err_msg=name)
    np.testing.assert_allclose(fm.w, r.w, rtol=rtol, atol=atol, err_msg=name)
    np.testing.assert_allclose(fm.intercept, r.b, rtol=rtol, atol=atol, err_msg=name)
    if zeros:
        assert np.array_equal(fm.P == 0.0, r.P == 0.0), name
    want = s.predict(R.Params(r.P.transpose(0, 2, 1), r.w, r.b))  # decisionFunction after fit
    np.testing.assert_allclose(fm.decisionFunction(X), want, rtol=1e-9, atol=1e-11, err_msg=name)


@pytest.mark.parametrize("name", ["pgd_sql12_deg2", "fista_restart", "nmapgd_sql12"])
def test_two_runs_are_bitwise_equal(name):
    a, oa, _, _ = device_fit(name)
    b, ob, _, _ = device_fit(name)
    assert np.array_equal(a.P, b.P) and np.array_equal(a.w, b.w) and a.intercept == b.intercept
    assert oa.iterations == ob.iterations


@pytest.mark.parametrize("name", ["fista_l21", "nmapgd_sql12"])
def test_warm_start_continues_the_state(name):
    algo, degree, fit_lower, fl, fi, skw, fkw = Cs.CASES[name]
    rtol, _ = tol_of(skw)
    whole, ow, _, _ = device_fit(name, max_iter=4)
    Xo, y, P0, w0, b0, n_aug = Cs.inputs(name)
    fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=P0.shape[1], fitLower=fit_lower, fitLinear=fl,
                                    fitIntercept=fi, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = device_opt(algo, skw, dict(fkw, max_iter=1))
    X = csr_of(Xo)
    seen = []
    for _ in range(4):
        opt.fit(X, y, fm)
        seen.append(opt.iterations[-1])
    assert [i["t"] for i in seen] == [i["t"] for i in ow.iterations]
    assert seen[-1]["t"] > 1.0
    if algo == "nmapgd":  # c and q are carried too; FISTA's accepted objective is not (fista.nim:97-98), so its later fits may differ
        assert [(i["c"], i["q"]) for i in seen] == [(i["c"], i["q"]) for i in ow.iterations]
        assert np.array_equal(fm.P, whole.P)


def test_callback_and_verbose_lines():
    name = "fista_restart"
    s, r = Cs.restate(name, verbose=1)
    seen = []
    out = io.StringIO()
    with redirect_stdout(out):
        fm, opt, _, _ = device_fit(name, verbose=1, callback=lambda o, m: seen.append((m.P.copy(), out.getvalue().count("\n"))))
    assert out.getvalue().splitlines() == r.lines
    cb = []
    Cs.restate(name, callback=lambda P, w, b: cb.append(P))
    assert len(seen) == len(cb)
    for q, ((P, lines_before), Pr) in enumerate(zip(seen, cb)):
        np.testing.assert_allclose(P, Pr, rtol=1e-10, atol=1e-14)  # the finalize()d model, restarts included
        assert lines_before == 1 + q  # the header and q verbose lines: the callback runs before its own iteration's line
    s, r = Cs.restate("pgd_converges", verbose=1)
    out = io.StringIO()
    with redirect_stdout(out):
        device_fit("pgd_converges", verbose=1)
    assert out.getvalue().splitlines() == r.lines and r.lines[-1].startswith("Converged at epoch")


def _create(L, mh, **kw):
    import ctypes as C
    c = dict(algo=0, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, rho=0.5, sigma=1.0, eta=0.5, loss=0, loss_param=1.0, reg=0,
             reg_transpose=0, max_search=-1)
    c.update(kw)
    h = C.c_void_p()
    rc = L.nfm_pgd_create(mh, c["algo"], c["alpha0"], c["alpha"], c["beta"], c["gamma"], c["rho"], c["sigma"], c["eta"], c["loss"],
                          c["loss_param"], c["reg"], c["reg_transpose"], c["max_search"], C.byref(h))
    return rc, h


def test_refusals():
    import ctypes as C
    L = capi.lib()
    Xo, _, y = make_fm_dataset(20, 6, 3, 4, 1)
    X = csr_of(Xo)

    def create(fm, **kw):
        fm.init(X)
        rc, h = _create(L, fm._push(X.ctx), **kw)
        if rc == 0:
            L.nfm_opt_destroy(h)
        return rc

    fm3 = nf.newFactorizationMachine("regression", degree=3, nComponents=4)
    fm2 = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    assert create(fm3, reg=capi.REG["squaredl12"], reg_transpose=1) == capi.ERR_INVALID
    assert create(fm3, reg=capi.REG["squaredl21"]) == capi.ERR_INVALID
    assert create(fm2, reg=capi.REG["omegati"]) == capi.ERR_UNSUPPORTED
    assert create(fm2, rho=1.0) == capi.ERR_INVALID and create(fm2, rho=0.0) == capi.ERR_INVALID
    assert create(fm2, reg=capi.REG["squaredl21"], reg_transpose=1) == capi.ERR_UNSUPPORTED
    assert create(fm2) == 0
    with pytest.raises(ValueError):
        nf.newPGD(reg=nf.newOmegaTI())
    # a field-aware model: ValueError from the Python host, NFM_ERR_UNSUPPORTED from the C ABI itself
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=2)
    with pytest.raises(ValueError):
        nf.newNMAPGD(verbose=0).fit(X, y, ffm)
    n, d, F = 8, 6, 3
    rng = np.random.default_rng(0)
    idx = np.stack([np.sort(rng.choice(d, 3, replace=False)) for _ in range(n)]).astype(np.int64)
    Xf = nf.newCSRFieldDataset(rng.uniform(-1, 1, n * 3), idx.ravel(), np.arange(n + 1, dtype=np.int64) * 3, (idx % F).ravel(), n, d, F)
    ffm.init(Xf)
    rc, _ = _create(L, ffm._push(Xf.ctx))
    assert rc == capi.ERR_UNSUPPORTED
    # the epoch call's rules, as CD's handle has them
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    opt = nf.newPGD(maxIter=1, verbose=0, reg=nf.newL1())
    opt.fit(X, y, fm)
    ls, vs = C.c_double(0), C.c_double(0)
    n = X.nSamples
    perm = np.arange(n, dtype=np.int64)
    assert L.nfm_opt_epoch(opt._h, X.h, perm.ctypes.data_as(C.c_void_p), 0, n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, n - 1, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, n, C.byref(ls), C.byref(vs)) == 0
    assert L.nfm_opt_set_shuffle(opt._h, 1) == capi.ERR_UNSUPPORTED
    assert L.nfm_opt_set_touch_cap(opt._h, 2.0) == capi.ERR_UNSUPPORTED
    # a data-parallel group: a real one-rank group handle is refused
    ctxs = (C.c_void_p * 1)(X.ctx.h.value)
    grp = (C.c_void_p * 1)()
    assert L.nfm_dp_create_local(ctxs, 1, grp) == 0
    try:
        assert L.nfm_opt_set_dp(opt._h, grp[0], 0, 0) == capi.ERR_UNSUPPORTED
    finally:
        L.nfm_dp_destroy(grp[0])
    # no begin_fit on this dataset: another dataset, and the same dataset after its targets changed
    X2 = csr_of(Xo)
    X2.set_targets(y)
    assert L.nfm_opt_epoch(opt._h, X2.h, None, 0, n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    X.set_targets(y + 1.0)
    assert L.nfm_opt_epoch(opt._h, X.h, None, 0, n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    fresh = nf.newFactorizationMachine("regression", degree=2, nComponents=4)
    fresh.init(X)
    rc, h = _create(L, fresh._push(X.ctx))
    assert rc == 0
    assert L.nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID  # never begun
    L.nfm_opt_destroy(h)
    # a repeated column id in a row
    Xr = nf.newCSRDataset(np.ones(4), np.array([0, 0, 1, 2]), np.array([0, 2, 4]), 2, 6)
    with pytest.raises(capi.NfmError) as ei:
        nf.newPGD(maxIter=1, verbose=0, reg=nf.newL1()).fit(Xr, np.zeros(2), nf.newFactorizationMachine("regression", nComponents=2))
    assert ei.value.code == capi.ERR_UNSUPPORTED


def _generic_parity(algo, Xo, y, degree, k, fit_lower, reg, rtol, max_iter=3, scale=0.05, **skw):
    fl = fi = True
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fl, seed=5, scale=scale)
    fm = nf.newFactorizationMachine("regression", degree=degree, nComponents=k, fitLower=fit_lower, warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = device_opt(algo, dict(reg=reg, **skw), dict(max_iter=max_iter, tol=0.0))
    opt.fit(csr_of(Xo), y, fm)
    s = R.Solver(algo, Xo, y, degree, n_aug, fl, fi, reg=reg, **skw)
    r = s.fit(P0, w0, b0, max_iter=max_iter, tol=0.0)
    worst = min(abs(a - b) / max(abs(a), abs(b)) for a, b in r.margins if np.isfinite(a) and np.isfinite(b) and max(abs(a), abs(b)) > 0)
    assert worst >= 1e-6, worst  # a condition on the input, as for the fixed cases
    assert [(i["trials"], i["branch"]) for i in opt.iterations] == [(tuple(i["trials"]), i["branch"]) for i in r.iters]
    print("max |dP| %.3e of %.3e" % (np.abs(fm.P - r.P).max(), np.abs(r.P).max()))
    np.testing.assert_allclose(fm.P, r.P, rtol=rtol, atol=rtol * 1e-2 * np.abs(r.P).max())
    np.testing.assert_allclose(fm.w, r.w, rtol=rtol, atol=rtol * 1e-2)
    return fm, r


def test_wide_model():
    Xo = random_csr(200, 40, 6, 3)
    y = np.random.default_rng(1).standard_normal(200)
    _generic_parity("nmapgd", Xo, y, 2, 130, "explicit", "l1", 1e-10, gamma=1e-4)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=130)
    with pytest.raises(capi.NfmError):
        nf.newPGD(maxIter=1, verbose=0, reg=nf.newL21()).fit(csr_of(Xo), y, fm)


def test_augment_at_degree_three():
    Xo, _, y = make_fm_dataset(80, 12, 3, 4, 11, "augment", True, True, threshold=0.4)
    _generic_parity("fista", Xo, y, 3, 4, "augment", "l21", 1e-10, gamma=1e-3, scale=0.2)


def test_segment_path_of_the_gradient():
    """feature 0 occurs in every one of 400 rows: more than 128 touches, so the column phase walks it in segments"""
    rng = np.random.default_rng(4)
    n, d, m = 400, 50, 5
    idx = np.stack([np.concatenate([[0], 1 + np.sort(rng.choice(d - 1, m - 1, replace=False))]) for _ in range(n)]).astype(np.int64)
    import oracle as O
    Xo = O.Dataset(np.arange(n + 1, dtype=np.int64) * m, idx.ravel(), rng.uniform(-1, 1, n * m), n, d)
    y = rng.standard_normal(n)
    _generic_parity("pgd", Xo, y, 2, 8, "explicit", "squaredl12", 1e-9, gamma=1e-3)


def _large_fit(name):
    shape, algo, skw, iters, scale = G.PGD_CASES[name]
    Xo, y, P0, w0, b0, n_aug = G.pgd_inputs(name)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=P0.shape[1], warmStart=True)
    fm.set_params(P0, w0, b0)
    opt = device_opt(algo, skw, dict(max_iter=iters, tol=0.0))
    opt.fit(csr_of(Xo), y, fm)
    return fm, opt


@pytest.mark.parametrize("name", list(G.PGD_CASES))
def test_large_grids(name):
    """the inputs of tests/dense_grid_cases.py: more than one workgroup per device block, a second and third trip of the row
    loops with a partial last wavefront, more than 64 partials per sum, the flat loops' second trip, and the row-parallel
    threshold passes reached from a line-search trial (tests/test_dense_grid_cases.py asserts that the shapes still get
    there, and bounds the restatement's own spread on them by a tenth of the tolerances used here)"""
    algo, skw = G.PGD_CASES[name][1:3]
    rtol, zeros = tol_of(skw)
    fm, opt = _large_fit(name)
    s, r = G.pgd_restate(name)
    check_iterations(name, opt, r, rtol, algo)
    atol = rtol * np.abs(r.P).max() * 1e-2
    print("%s max |dP| %.3e of %.3e max |dw| %.3e |db| %.3e" % (name, np.abs(fm.P - r.P).max(), np.abs(r.P).max(), np.abs(fm.w - r.w).max(),
                                                               abs(fm.intercept - r.b)))
    np.testing.assert_allclose(fm.P, r.P, rtol=rtol, atol=atol, err_msg=name)
    np.testing.assert_allclose(fm.w, r.w, rtol=rtol, atol=atol, err_msg=name)
    np.testing.assert_allclose(fm.intercept, r.b, rtol=rtol, atol=atol, err_msg=name)
    if zeros:
        assert np.array_equal(fm.P == 0.0, r.P == 0.0), name
    if name in G.PGD_BITWISE:
        again, oa = _large_fit(name)
        assert np.array_equal(fm.P, again.P) and np.array_equal(fm.w, again.w) and fm.intercept == again.intercept
        assert opt.iterations == oa.iterations
