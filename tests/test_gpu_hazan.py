"""newConvexFactorizationMachine and newHazan on the device against the restatement of the reference
(tests/hazan_restatement.py) on the fixed cases of tests/hazan_cases.py.

Tolerances are the reference's own (tests/test_hazan.nim, checkAlmostEqual): P and w at rtol 1e-6 / atol 1e-9, lams at atol
1e-7, the intercept at 1e-5 absolute; the records' loss and step size at 1e-8 relative.  The discrete stops (the power
method's, CG's, the nTol rule) flip under rounding, so parity runs switch them off (tolPower = 0, tol = -100) or force the
restatement to the device's counts after checking the counts themselves; the stops have tests of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hazan_cases as hc
import hazan_restatement as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nf():
    import __graft_entry__ as g
    g.build()
    import nimfm_amd
    return nimfm_amd


def _dataset(nf, X):
    return nf.newCSRDataset(X.rval, X.ridx, X.rptr, X.n, X.d)


def _close(got, want, rtol=1e-6, atol=1e-9):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


def _check_model(cfm, ref):
    assert cfm.P.shape == ref.P.shape
    _close(cfm.P, ref.P)
    _close(cfm.w, ref.w)
    _close(cfm.lams, ref.lams, rtol=0.0, atol=1e-7)
    assert abs(cfm.intercept - ref.intercept) < 1e-5


def _check_records(hist, ref_hist):
    assert len(hist) == len(ref_hist)
    for got, want in zip(hist, ref_hist):
        for key in ("slot", "nComponents", "powerIters", "cgIters"):
            assert got[key] == want[key], (key, got, want)
        for key in ("loss", "step"):
            assert abs(got[key] - want[key]) <= 1e-8 * abs(want[key]), (key, got[key], want[key])


def _kw(shape, optimal, ignoreDiag, fitLinear, fitIntercept, **over):
    kw = dict(maxComponents=shape["maxComponents"], ignoreDiag=ignoreDiag, fitLinear=fitLinear, fitIntercept=fitIntercept,
              maxIter=shape["maxIter"], eta=shape["eta"], tol=shape["tol"], maxIterPower=shape["maxIterPower"],
              tolPower=shape["tolPower"], optimal=optimal)
    kw.update(over)
    return kw


def _device_fit(nf, X, y, kw, powerInit=None, cfm=None, opt=None, task="regression", warmStart=False, verbose=0, callback=None):
    cfm = cfm or nf.newConvexFactorizationMachine(task, maxComponents=kw["maxComponents"], fitIntercept=kw["fitIntercept"],
                                                  fitLinear=kw["fitLinear"], ignoreDiag=kw["ignoreDiag"], warmStart=warmStart)
    opt = opt or nf.newHazan(maxIter=kw["maxIter"], eta=kw["eta"], verbose=verbose, tol=kw["tol"], nTol=kw.get("nTol", 10),
                             maxIterPower=kw["maxIterPower"], tolPower=kw["tolPower"], optimal=kw["optimal"])
    opt.fit(_dataset(nf, X), y, cfm, callback=callback, powerInit=powerInit)
    return cfm, opt


@pytest.mark.parametrize("optimal,ignoreDiag,fitLinear,fitIntercept", hc.grid_flags())
def test_reference_grid(nf, optimal, ignoreDiag, fitLinear, fitIntercept):
    """n = 50, d = 6, maxComponents = 6: after randomize(1) on both sides the start vectors come from the same stream"""
    X, y = hc.grid_data(fitLinear, fitIntercept)
    kw = _kw(hc.GRID, optimal, ignoreDiag, fitLinear, fitIntercept)
    nf.randomize(1)
    cfm, opt = _device_fit(nf, X, y, kw)
    forced = [(r["powerIters"], r["cgIters"]) for r in opt.history]
    plain = hr.hazan_fit(X, y, hc.nim_starts(1, kw["maxIter"], X.d), **kw)
    for got, want in zip(opt.history, plain.history):  # the CG stop is live: its count may differ by one at a thin margin
        assert abs(got["cgIters"] - want["cgIters"]) <= 1, (got, want)
    ref = hr.hazan_fit(X, y, hc.nim_starts(1, kw["maxIter"], X.d), forced=forced, **kw)
    _check_model(cfm, ref)
    _check_records(opt.history, ref.history)
    assert opt.it == ref.it
    if not optimal:
        assert len(opt.history) == kw["maxComponents"] < kw["maxIter"]  # the early break of optimal = false
    else:
        assert any(r["slot"] < i for i, r in enumerate(opt.history) if i >= kw["maxComponents"])  # the replace branch ran


@pytest.fixture(scope="module")
def wide():
    return hc.wide_data()


@pytest.mark.parametrize("ignoreDiag,optimal,fitLinear,fitIntercept", hc.WIDE_RUNS)
def test_wide_case(nf, wide, ignoreDiag, optimal, fitLinear, fitIntercept):
    """n = 2500, d = 300: more than one workgroup in every pass, a column that holds every sample, a row of 200 entries, an
    empty row and an empty column; the CG stop is live"""
    X, y = wide
    kw = _kw(hc.WIDE, optimal, ignoreDiag, fitLinear, fitIntercept)
    starts = hc.numpy_starts(100)
    outer = iter(range(kw["maxIter"]))
    cfm, opt = _device_fit(nf, X, y, kw, powerInit=lambda d: starts(next(outer), d))
    plain = hr.hazan_fit(X, y, starts, **kw)
    assert len(opt.history) == len(plain.history)
    for got, want in zip(opt.history, plain.history):
        print("cg iterations: device %d, restatement %d (||r||_1 / tol at its stop %.3g, one earlier %.3g)"
              % (got["cgIters"], want["cgIters"], want["cgNorm"] / want["cgTol"] if want["cgTol"] else 0.0,
                 want["cgNormPrev"] / want["cgTol"] if want["cgTol"] else 0.0))
        assert abs(got["cgIters"] - want["cgIters"]) <= 1, (got, want)
    forced = [(r["powerIters"], r["cgIters"]) for r in opt.history]
    ref = hr.hazan_fit(X, y, starts, forced=forced, **kw)
    _check_model(cfm, ref)
    _check_records(opt.history, ref.history)
    for got, want in zip(opt.history, plain.history):  # a margin of 2x on both sides of the stop: the counts are equal
        if want["cgTol"] > 0 and 2 * want["cgNorm"] <= want["cgTol"] and want["cgNormPrev"] >= 2 * want["cgTol"]:
            assert got["cgIters"] == want["cgIters"], (got, want)
    if fitLinear:
        assert max(r["cgIters"] for r in opt.history) > 1
    else:
        assert not cfm.w.any() and cfm.intercept == 0.0


def test_power_stop(nf):
    """tolPower = 1e-7 on the tiny grid: where the restatement's |eval - evalOld| is below tolPower / 2 at its stop and above
    2 tolPower one iteration earlier, the device stops at the same count"""
    margins = 0
    for optimal, ignoreDiag, fitLinear, fitIntercept in hc.POWER_STOP_FLAGS:
        X, y = hc.grid_data(fitLinear, fitIntercept, scales=hc.POWER_STOP_SCALES)
        kw = _kw(hc.GRID, optimal, ignoreDiag, fitLinear, fitIntercept, tolPower=1e-7, maxIter=3)
        starts = hc.numpy_starts(300)
        outer = iter(range(kw["maxIter"]))
        cfm, opt = _device_fit(nf, X, y, kw, powerInit=lambda d: starts(next(outer), d))
        ref = hr.hazan_fit(X, y, starts, **kw)
        for got, want in zip(opt.history, ref.history):
            print("power iterations: device %d, restatement %d (diff %.3g, one earlier %.3g)"
                  % (got["powerIters"], want["powerIters"], want["powerDiff"], want["powerDiffPrev"]))
            if want["powerDiff"] < 1e-7 / 2 and want["powerDiffPrev"] > 2e-7 and want["powerIters"] < kw["maxIterPower"]:
                margins += 1
                assert got["powerIters"] == want["powerIters"], (got, want)
            elif got["powerIters"] != want["powerIters"]:
                break  # a thin margin flipped the stop: the two runs part here
    assert margins >= 1


def test_ntol_rule(nf, capsys):
    X, y = hc.grid_data(True, True)
    kw = _kw(hc.GRID, True, True, True, True, tol=1e9, nTol=4, maxIter=9)
    nf.randomize(1)
    cfm, opt = _device_fit(nf, X, y, kw, verbose=1)
    assert len(opt.history) == 4 and opt.it == 3  # not incremented on the converging iteration
    out = capsys.readouterr().out
    assert "Converged at iteration 4." in out and "did not converge" not in out
    kw = _kw(hc.GRID, True, True, True, True, tol=-100.0, maxIter=3)
    cfm, opt = _device_fit(nf, X, y, kw, verbose=1)
    out = capsys.readouterr().out
    assert len(opt.history) == 3 and opt.it == 3
    assert out.rstrip().endswith("Objective did not converge. Increase maxIter.")
    lines = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(lines) == 3 and lines[0].startswith("Epoch: 0   MSE/2: ") and "   Trace Norm: " in lines[0]
    assert lines[2] == "Epoch: 2   MSE/2: %1.4e   Trace Norm: %1.4e" % (opt.history[2]["loss"] / 2.0, opt.history[2]["trace"])


@pytest.mark.parametrize("optimal", [True, False])
def test_warm_start(nf, optimal):
    """N fits of one iteration on a warm-start model equal one fit of N iterations; self.it is carried across the fits"""
    X, y = hc.grid_data(True, True)
    N = 5
    kw = _kw(hc.GRID, optimal, True, True, True, maxIter=N)
    nf.randomize(1)
    cold, opt_cold = _device_fit(nf, X, y, kw)
    nf.randomize(1)
    kw1 = dict(kw, maxIter=1)
    warm = nf.newConvexFactorizationMachine("regression", maxComponents=kw["maxComponents"], warmStart=True)
    opt = nf.newHazan(maxIter=1, eta=kw["eta"], verbose=0, tol=kw["tol"], maxIterPower=kw["maxIterPower"], tolPower=0.0, optimal=optimal)
    ds = _dataset(nf, X)
    for i in range(N):
        opt.fit(ds, y, warm)
        assert opt.it == i + 1
    assert kw1["maxIter"] == 1 and opt_cold.it == N
    assert abs(cold.intercept - warm.intercept) < 1e-5
    _close(warm.w, cold.w)
    _close(warm.lams, cold.lams, rtol=0.0, atol=1e-7)
    _close(warm.P, cold.P)


def test_two_runs_are_bitwise_equal(nf, wide):
    X, y = wide
    kw = _kw(hc.WIDE, True, True, True, True, maxIter=3)
    runs = []
    for _ in range(2):
        starts, outer = hc.numpy_starts(100), iter(range(3))
        cfm, opt = _device_fit(nf, X, y, kw, powerInit=lambda d: starts(next(outer), d))
        runs.append((cfm.P.copy(), cfm.lams.copy(), cfm.w.copy(), cfm.intercept, [tuple(sorted(r.items())) for r in opt.history]))
    a, b = runs
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("task", ["regression", "classification"])
@pytest.mark.parametrize("ignoreDiag", [True, False])
def test_decision_function_against_numpy(nf, wide, task, ignoreDiag):
    X, _ = wide  # row 7 is longer than a wavefront, row 11 is empty
    rng = np.random.default_rng(5)
    Xd = X.dense()
    ds = _dataset(nf, X)
    cfm = nf.newConvexFactorizationMachine(task, maxComponents=4, ignoreDiag=ignoreDiag)
    w = rng.normal(size=X.d)
    cfm.set_params(np.zeros((0, X.d)), np.zeros(0), w, 0.25)  # zero components: intercept + <w, x>
    _close(cfm.decisionFunction(ds), Xd @ w + 0.25, rtol=1e-12, atol=1e-12)
    P, lams = rng.normal(size=(3, X.d)), np.array([0.5, -1.5, 2.0])
    cfm.set_params(P, lams, w, 0.25)
    want = Xd @ w + 0.25
    for s in range(3):
        a = Xd @ P[s]
        want += lams[s] * (0.5 * (a * a - (Xd * Xd) @ (P[s] * P[s])) if ignoreDiag else a * a)
    got = cfm.decisionFunction(ds)
    _close(got, want, rtol=1e-11, atol=1e-11)
    _close(got, hr.decision_function(X, P, lams, w, 0.25, ignoreDiag), rtol=1e-13, atol=1e-13)
    assert (cfm.predict(ds) == np.sign(got)).all()
    _close(cfm.predictProba(ds), nf.expit(got), rtol=1e-12, atol=0)
    y = np.sign(want) if task == "classification" else want + 0.1
    score = cfm.score(ds, y)
    if task == "classification":
        assert score == pytest.approx(float(np.mean(np.sign(got) == y)))
    else:
        assert score == pytest.approx(float(np.sqrt(np.mean((got - y) ** 2))), rel=1e-10)
    m = cfm.metrics(ds, y)
    assert set(m) == {"rmse", "accuracy", "rocauc"}


def test_classification_fit_and_public_paths(nf, tmp_path, capsys):
    """checkTarget maps the targets to +-1; score, dump -> load -> the same predictions, the callback, the verbose lines"""
    X, y = hc.grid_data(True, True)
    yc = np.where(y > np.median(y), 3.0, -2.0)
    kw = _kw(hc.GRID, True, True, True, True, maxIter=4)
    seen = []
    nf.randomize(1)
    cfm, opt = _device_fit(nf, X, yc, kw, task="classification", verbose=2,
                           callback=lambda o, m: seen.append((o.it, m.nComponents, m.lams.copy())))
    ref = hr.hazan_fit(X, yc, hc.nim_starts(1, 4, X.d), task="classification", forced=[(r["powerIters"], r["cgIters"]) for r in opt.history], **kw)
    _check_model(cfm, ref)
    assert [s[:2] for s in seen] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch:")]) == 4
    ds = _dataset(nf, X)
    assert cfm.score(ds, yc) == pytest.approx(float(np.mean(np.sign(cfm.decisionFunction(ds)) == np.sign(yc))))
    path = str(tmp_path / "cfm.txt")
    cfm.dump(path)
    back = nf.load(path, False, ignoreDiag=True)
    assert isinstance(back, nf.ConvexFactorizationMachine) and back.maxComponents == 6 and back.nComponents == 4
    assert back.decisionFunction(ds).tobytes() == cfm.decisionFunction(ds).tobytes()


def test_command_line(nf, tmp_path):
    X, y = hc.grid_data(True, True)
    Xd = X.dense()
    train = tmp_path / "train.svm"
    with open(train, "w") as f:
        for i in range(X.n):
            f.write("%r %s\n" % (float(y[i]), " ".join("%d:%r" % (j + 1, float(Xd[i, j])) for j in range(X.d) if Xd[i, j] != 0.0)))
    dump = tmp_path / "model.txt"
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    base = [sys.executable, "-m", "nimfm_amd"]
    out = subprocess.run(base + ["train", "-t", "r", "--train", str(train), "--test", str(train), "--solver", "hazan", "--maxComponents", "4",
                                 "--eta", "3.0", "--maxIterPower", "50", "--ignoreDiag", "true", "--maxIter", "6", "--dump", str(dump),
                                 "--nFeatures", "6"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Test RMSE: " in out.stdout and "Epoch: " in out.stdout
    assert open(dump).read().splitlines()[4] == "maxComponents: 4"
    out2 = subprocess.run(base + ["test", "-t", "r", "--test", str(train), "--load", str(dump), "--nFeatures", "6", "--ignoreDiag", "true"],
                          capture_output=True, text=True, env=env, timeout=300)
    assert out2.returncode == 0, out2.stdout + out2.stderr
    rm = [l for l in out.stdout.splitlines() if l.startswith("Test RMSE")][0]
    assert rm in out2.stdout
    out3 = subprocess.run(base + ["train", "-t", "r", "--train", str(train), "--solver", "gcd"], capture_output=True, text=True, env=env, timeout=300)
    assert out3.returncode != 0 and "gcd" in out3.stderr and "nimfm_cfm" in out3.stderr


def test_refusals(nf):
    X, y = hc.grid_data(True, True)
    ds = _dataset(nf, X)
    fm = nf.newFactorizationMachine("regression", nComponents=2)
    with pytest.raises(ValueError, match="ConvexFactorizationMachine"):
        nf.newHazan(verbose=0).fit(ds, y, fm)
    with pytest.raises(ValueError, match="maxComponents < 1."):
        nf.newConvexFactorizationMachine("regression", maxComponents=0)
    for make in (nf.newSGD, nf.newAdaGrad, nf.newCD, nf.newPCD, nf.newPBCD, nf.newMBPSGD, nf.newPGD, nf.newFISTA, nf.newNMAPGD, nf.newKatyusha):
        with pytest.raises(ValueError, match="ConvexFactorizationMachine"):
            make(verbose=0).fit(ds, y, nf.newConvexFactorizationMachine("regression"))
    # the C ABI refuses too
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=2)
    cfm.init(ds)
    import ctypes as C
    from nimfm_amd import _capi as capi
    h = C.c_void_p()
    assert capi.lib().nfm_cd_create(cfm._push(ds.ctx), 1e-6, 1e-3, 1e-3, 0, 1.0, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert capi.lib().nfm_hazan_create(fm._handle(ds.ctx) if fm._d else _init(fm, ds), 1000.0, 10, 1e-7, 1, C.byref(h)) == capi.ERR_UNSUPPORTED
    # a dataset with the wrong nFeatures
    kw = _kw(hc.GRID, True, True, True, True, maxIter=1)
    nf.randomize(1)
    fitted, _ = _device_fit(nf, X, y, kw)
    wrong = nf.newCSRDataset(X.rval, X.ridx, X.rptr, X.n, X.d + 1)
    with pytest.raises(ValueError, match="Invalid nFeatures."):
        fitted.decisionFunction(wrong)
    warm = nf.newConvexFactorizationMachine("regression", maxComponents=6, warmStart=True)
    opt = nf.newHazan(maxIter=1, eta=3.0, verbose=0, maxIterPower=20)
    opt.fit(ds, y, warm)
    with pytest.raises(ValueError, match="Invalid nFeatures."):
        opt.fit(wrong, y, warm)
    # a repeated column id in a row
    rep = nf.newCSRDataset(np.array([1.0, 2.0, 3.0]), np.array([0, 0, 1]), np.array([0, 2, 3]), 2, 6)
    with pytest.raises(nf.NfmError, match="repeated column ids"):
        nf.newHazan(maxIter=1, verbose=0).fit(rep, np.array([1.0, 2.0]), nf.newConvexFactorizationMachine("regression"))


def _init(fm, ds):
    fm.init(ds)
    return fm._push(ds.ctx)
