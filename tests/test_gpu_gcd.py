"""newGreedyCD on the device against the restatement of the reference (tests/gcd_restatement.py) on the fixed cases of
tests/gcd_cases.py.

Tolerances are tests/test_gpu_hazan.py's: P and w at rtol 1e-6 / atol 1e-9, lams at atol 1e-7, the intercept at 1e-5 absolute,
the records' objectives at 1e-8 relative; tests/test_gcd_restatement.py guards that rounding moves every case at least 100x
less.  The discrete stops flip under rounding, so parity runs switch them off (tolPower = 0, tol = 0) or force the restatement
to the device's counts after checking the counts themselves."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gcd_cases as gc
import gcd_restatement as gr
import hazan_cases as hc
import hazan_restatement as hr

pytestmark = pytest.mark.gpu
T = gc.TOL


@pytest.fixture(scope="module")
def nf():
    import __graft_entry__ as g
    g.build()
    import nimfm_amd
    return nimfm_amd


def _dataset(nf, X):
    return nf.newCSRDataset(X.rval, X.ridx, X.rptr, X.n, X.d)


def _device_fit(nf, X, y, kw, cfm=None, verbose=0, callback=None, powerInit=None, seed=1, **over):
    kw = dict(kw, **over)
    cfm = cfm or nf.newConvexFactorizationMachine(kw.get("task", "regression"), maxComponents=kw["maxComponents"], fitIntercept=kw["fitIntercept"],
                                                  fitLinear=kw["fitLinear"], ignoreDiag=kw["ignoreDiag"])
    opt = nf.newGreedyCD(maxIter=kw["maxIter"], alpha0=kw["alpha0"], alpha=kw["alpha"], beta=kw["beta"], loss=kw.get("loss", "squared"),
                         maxIterInner=kw["maxIterInner"], nRefitting=kw["nRefitting"], verbose=verbose, tol=kw["tol"],
                         maxIterPower=kw["maxIterPower"], tolPower=kw["tolPower"])
    if seed is not None:
        nf.randomize(seed)
    opt.fit(_dataset(nf, X), y, cfm, callback=callback, powerInit=powerInit)
    return cfm, opt


@functools.lru_cache(maxsize=None)
def _reference(name, forced_key):
    """the restatement of one case, forced to the device's discrete decisions; computed once per (case, decisions)"""
    X, y, kw = gc.case(name)
    forced = None if forced_key is None else dict(power=list(forced_key[0]), inner=list(forced_key[1]), outer=forced_key[2])
    return gr.gcd_fit(X, y, gc.starts(64, X.d), summation="tree", forced=forced, **kw)


def _key(counts):
    return (tuple(counts["power"]), tuple(counts["inner"]), counts["outer"])


def _inner(history):
    return [r for o in history for r in o["inner"]]


def _check_model(name, cfm, ref):
    keep = ref.P.shape[0] - gc.DROP_P_ROWS.get(name, 0)
    assert cfm.P.shape == ref.P.shape and len(cfm.lams) == len(ref.lams)
    dP = np.abs(cfm.P - ref.P)[:keep]
    print("%s: max |dP| %.3e  |dw| %.3e  |dlams| %.3e  |db| %.3e" % (name, dP.max() if dP.size else 0.0, np.abs(cfm.w - ref.w).max(),
                                                                  np.abs(cfm.lams - ref.lams).max() if len(ref.lams) else 0.0,
                                                                  abs(cfm.intercept - ref.intercept)))
    np.testing.assert_allclose(cfm.P[:keep], ref.P[:keep], rtol=T["P_rtol"], atol=T["P_atol"])
    np.testing.assert_allclose(cfm.w, ref.w, rtol=T["w_rtol"], atol=T["w_atol"])
    np.testing.assert_allclose(cfm.lams, ref.lams, rtol=0.0, atol=T["lams_atol"])
    assert abs(cfm.intercept - ref.intercept) < T["intercept_atol"]


def _check_records(hist, ref_hist):
    assert len(hist) == len(ref_hist)
    for got, want in zip(hist, ref_hist):
        assert got["nComponents"] == want["nComponents"] and len(got["inner"]) == len(want["inner"])
        for key in ("loss", "reg", "objOld"):
            assert abs(got[key] - want[key]) <= T["obj_rtol"] * abs(want[key]), (key, got[key], want[key])
        for g, w in zip(got["inner"], want["inner"]):
            for key in ("added", "slot", "powerIters", "nComponents", "nStored", "refit", "checked"):
                assert g[key] == w[key], (key, g, w)
            assert abs(g["objective"] - w["objective"]) <= T["obj_rtol"] * abs(w["objective"]), (g, w)
            assert abs(g["lam"] - w["lam"]) <= T["lams_atol"]
            if w["slot"] >= 0:
                assert abs(g["eval"] - w["eval"]) <= 1e-6 * abs(w["eval"]) + 1e-9


def _run_case(nf, name, within_one=False):
    X, y, kw = gc.case(name)
    cfm, opt = _device_fit(nf, X, y, kw)
    counts = gr.counts_of(opt.history)
    if within_one:  # the stops are live: against the unforced restatement every count is within one
        plain = gr.counts_of(_reference(name, None).history)
        print("%s: device counts %s, restatement %s" % (name, counts, plain))
        assert counts["outer"] == plain["outer"] or abs(counts["outer"] - plain["outer"]) <= 1
        for a, b in zip(counts["power"], plain["power"]):
            assert abs(a - b) <= 1
            if a != b:
                break  # the two runs part here
    ref = _reference(name, _key(counts))
    _check_model(name, cfm, ref)
    _check_records(opt.history, ref.history)
    return cfm, opt, ref, kw


@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_reference_grid(nf, name):
    """n = 50, d = 6, maxComponents = 6, squared loss: after randomize(1) the start vectors come from the same stream"""
    cfm, opt, ref, kw = _run_case(nf, name)
    if not kw["fitLinear"]:
        assert not cfm.w.any()
    if not kw["fitIntercept"]:
        assert cfm.intercept == 0.0
    assert cfm.nComponents == 6 and gr.counts_of(opt.history)["power"] == [1000] * 6


@pytest.mark.parametrize("name", gc.LOSS_CASES)
def test_other_losses_as_classification(nf, name):
    cfm, opt, ref, kw = _run_case(nf, name)
    assert kw["task"] == "classification" and kw["loss"] != "squared"


@pytest.mark.parametrize("name", gc.WIDE_CASES)
def test_wide_case(nf, name):
    """n = 2500, d = 300: more than one workgroup in every pass, more than one level in the w sweep, partial-sum trees wider than
    one block, a column that holds every sample, a row of 200 entries, an empty row and an empty column"""
    cfm, opt, ref, kw = _run_case(nf, name)
    assert any(r["refit"] for r in _inner(opt.history)) and cfm.nComponents == 3
    if not kw["fitLinear"]:
        assert not cfm.w.any()


def test_branch_threshold_and_slot_reuse(nf):
    for name in ("branch:big_beta", "branch:refit1"):
        cfm, opt, ref, kw = _run_case(nf, name)
        recs = _inner(opt.history)
        k = next(i for i, r in enumerate(recs) if r["slot"] >= 0 and not r["added"])
        assert recs[k]["lam"] == 0.0 and recs[k]["nStored"] > recs[k]["nComponents"]  # stored, not counted
        nxt = next(r for r in recs[k + 1:] if r["slot"] >= 0)
        assert nxt["slot"] == recs[k]["slot"] and nxt["nStored"] == recs[k]["nStored"]  # re-used, not appended
        dropped = False  # refitDiag drove a component to zero
        for o in opt.history:
            before = o["nComponentsStart"]
            for r in o["inner"]:
                dropped = dropped or (r["refit"] and r["nComponents"] < before + r["added"])
                before = r["nComponents"]
        assert dropped


def test_branch_full_basis(nf):
    cfm, opt, ref, kw = _run_case(nf, "branch:full_basis")
    recs = _inner(opt.history)
    assert sum(r["slot"] >= 0 for r in recs) == 2 and any(r["slot"] < 0 and r["powerIters"] == 0 for r in recs)
    assert cfm.nComponents == 2


def test_branch_no_refit(nf):
    cfm, opt, ref, kw = _run_case(nf, "branch:norefit")
    assert not any(r["refit"] for r in _inner(opt.history))


def test_power_stop(nf):
    cfm, opt, ref, kw = _run_case(nf, "branch:power_stop", within_one=True)
    counts = gr.counts_of(opt.history)["power"]
    assert counts and all(1 < c < kw["maxIterPower"] for c in counts)
    assert counts == gr.counts_of(_reference("branch:power_stop", None).history)["power"]  # the CPU test holds the margins


def test_tol_stops(nf, capsys):
    X, y, kw = gc.case("branch:tol_stop")
    cfm, opt, ref, kw = _run_case(nf, "branch:tol_stop", within_one=True)
    plain = _reference("branch:tol_stop", None)
    assert gr.counts_of(opt.history) == gr.counts_of(plain.history)  # the CPU test holds the margins
    assert len(opt.history) < kw["maxIter"] and any(len(o["inner"]) < kw["maxIterInner"] for o in opt.history)
    capsys.readouterr()
    _device_fit(nf, X, y, kw, verbose=2)
    out = capsys.readouterr().out
    assert "Converged at iteration %d." % len(opt.history) in out and "   Converged at iteration " in out and "did not converge" not in out


@pytest.mark.parametrize("ignoreDiag,fitLinear,fitIntercept", gc.grid_flags())
def test_warm_start(nf, ignoreDiag, fitLinear, fitIntercept):
    """10 fits of one iteration on a warm-start model equal one fit of 10 iterations (tests/test_greedy_cd.nim:56-88)"""
    X, y = hc.grid_data(fitLinear, fitIntercept)
    ds = _dataset(nf, X)
    mk = dict(maxComponents=6, fitLinear=fitLinear, fitIntercept=fitIntercept, ignoreDiag=ignoreDiag)
    nf.randomize(1)
    warm = nf.newConvexFactorizationMachine("regression", warmStart=True, **mk)
    opt = nf.newGreedyCD(maxIter=1, verbose=0, tol=0)
    for i in range(10):
        opt.fit(ds, y, warm)
        if i == 0:
            first = warm.nComponents
        else:
            assert opt.history[0]["nComponentsStart"] > 0 and warm.nComponents >= first  # begins with components
    nf.randomize(1)
    cold = nf.newConvexFactorizationMachine("regression", **mk)
    nf.newGreedyCD(maxIter=10, verbose=0, tol=0).fit(ds, y, cold)
    assert abs(cold.intercept - warm.intercept) < 1e-5
    np.testing.assert_allclose(warm.w, cold.w, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(warm.lams, cold.lams, rtol=1e-6, atol=1e-9)


def test_two_runs_are_bitwise_equal(nf):
    X, y, kw = gc.case("wide:11")
    runs = []
    for _ in range(2):
        cfm, opt = _device_fit(nf, X, y, kw)
        runs.append((cfm.P.tobytes(), cfm.lams.tobytes(), cfm.w.tobytes(), cfm.intercept, repr(opt.history)))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("ignoreDiag,fitLinear,fitIntercept", [(True, True, True), (False, False, True), (True, True, False), (False, False, False)])
def test_score_improves(nf, ignoreDiag, fitLinear, fitIntercept):
    """tests/test_greedy_cd.nim:138-160"""
    X, y = hc.grid_data(fitLinear, fitIntercept)
    ds = _dataset(nf, X)
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=6, fitLinear=fitLinear, fitIntercept=fitIntercept, ignoreDiag=ignoreDiag)
    cfm.init(ds)
    before = cfm.score(ds, y)
    nf.randomize(1)
    nf.newGreedyCD(maxIter=20, verbose=0, tol=0, alpha0=1e-9, alpha=1e-9, beta=1e-9).fit(ds, y, cfm)
    assert cfm.score(ds, y) < before


@pytest.mark.parametrize("ignoreDiag", [True, False])
def test_strong_regularization_shrinks(nf, ignoreDiag):
    """tests/test_greedy_cd.nim:163-198, at n = 50"""
    X, y = hc.grid_data(True, True)
    ds = _dataset(nf, X)
    fits = []
    for a0, a, b in ((1e-5, 1e-5, 1e-6), (1e7, 1e7, 1e8)):
        cfm = nf.newConvexFactorizationMachine("regression", maxComponents=6, ignoreDiag=ignoreDiag)
        nf.randomize(1)
        nf.newGreedyCD(maxIter=100, verbose=0, tol=0, alpha0=a0, alpha=a, beta=b).fit(ds, y, cfm)
        fits.append(cfm)
    weak, strong = fits
    assert weak.score(ds, y) < strong.score(ds, y)
    assert abs(weak.intercept) >= abs(strong.intercept)
    assert np.linalg.norm(weak.w) >= np.linalg.norm(strong.w)
    assert np.linalg.norm(weak.lams) >= np.linalg.norm(strong.lams)


def test_public_paths_with_a_zero_slot(nf, tmp_path):
    """decisionFunction, score, dump -> load of a model that holds a component thresholded to zero"""
    X, y = hc.grid_data(True, True)
    ds = _dataset(nf, X)
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=4, warmStart=True)
    nf.randomize(1)
    nf.newGreedyCD(maxIter=1, maxIterInner=3, verbose=0, tol=0).fit(ds, y, cfm)
    assert cfm.nComponents == 3 and cfm.lams.all()
    opt = nf.newGreedyCD(maxIter=1, maxIterInner=1, beta=0.5, verbose=0, tol=0)
    opt.fit(ds, y, cfm)
    assert cfm.nComponents == 4 and cfm.lams[3] == 0.0 and cfm.lams[:3].all() and cfm.P[3].any()  # stored with its P row
    assert opt.history[0]["inner"][0]["slot"] == 3 and opt.history[0]["inner"][0]["added"] == 0
    got = cfm.decisionFunction(ds)
    np.testing.assert_allclose(got, hr.decision_function(X, cfm.P, cfm.lams, cfm.w, cfm.intercept, True), rtol=1e-13, atol=1e-13)
    assert cfm.score(ds, y) == pytest.approx(float(np.sqrt(np.mean((got - y) ** 2))), rel=1e-10)
    path = str(tmp_path / "cfm.txt")
    cfm.dump(path)
    lines = open(path).read().splitlines()
    assert lines[3] == "nComponents: 4" and lines[8].split(" ")[3] == "0.0"
    back = nf.load(path, True, ignoreDiag=True)
    assert back.nComponents == 4 and back.lams[3] == 0.0 and back.decisionFunction(ds).tobytes() == got.tobytes()
    nf.newGreedyCD(maxIter=1, maxIterInner=1, verbose=0, tol=0).fit(ds, y, back)  # the zero slot is the one used next
    assert back.nComponents == 4 and back.lams[3] != 0.0


def test_verbose_text_and_callback(nf, capsys):
    X, y, kw = gc.case("branch:full_basis")
    seen = []
    cfm, opt = _device_fit(nf, X, y, kw, verbose=1, callback=lambda o, m: seen.append((m.nComponents, m.lams.copy(), len(o.history))))
    out = capsys.readouterr().out.splitlines()
    want = []
    for i, o in enumerate(opt.history):
        want += ["Outer Iteration %d" % (i + 1), "   Loss: %1.4e   Reg: %1.4e" % (o["loss"], o["reg"])]
    want.append("Objective did not converge. Increase maxIter.")
    assert out == want
    assert [s[0] for s in seen] == [2, 2, 2] and [s[2] for s in seen] == [1, 2, 3] and (seen[-1][1] == cfm.lams).all()
    cfm, opt = _device_fit(nf, X, y, kw, verbose=2)
    out = capsys.readouterr().out.splitlines()
    want = []
    for i, o in enumerate(opt.history):
        want.append("Outer Iteration %d" % (i + 1))
        old = o["objOld"]
        for r in o["inner"]:
            if r["checked"]:
                want.append("   Iteration: %d   Objective: %1.4e   Decreasing: %1.4e" % (r["it"] + 1, r["objective"], old - r["objective"]))
                old = r["objective"]
        want.append("   Loss: %1.4e   Reg: %1.4e" % (o["loss"], o["reg"]))
    want.append("Objective did not converge. Increase maxIter.")
    assert out == want


def test_refusals(nf, tmp_path):
    from nimfm_amd import _capi as capi
    X, y = hc.grid_data(True, True)
    ds = _dataset(nf, X)
    with pytest.raises(ValueError, match="dsyev.*reference"):
        nf.newGreedyCD(refitFully=True, verbose=0).fit(ds, y, nf.newConvexFactorizationMachine("regression"))
    with pytest.raises(ValueError, match="nRefitting"):
        nf.newGreedyCD(nRefitting=0)
    fm = nf.newFactorizationMachine("regression", nComponents=2)
    with pytest.raises(ValueError, match="ConvexFactorizationMachine"):
        nf.newGreedyCD(verbose=0).fit(ds, y, fm)
    with pytest.raises(ValueError, match="newGreedyCD"):
        nf.newCD(verbose=0).fit(ds, y, nf.newConvexFactorizationMachine("regression"))
    # the C ABI: GreedyCD refuses every other model kind, the other optimizers' entries refuse GreedyCD's handle
    L = capi.lib()
    h = C.c_void_p()
    fm.init(ds)
    assert L.nfm_gcd_create(fm._push(ds.ctx), 1e-6, 1e-3, 1e-5, 0, 1.0, 100, 1e-7, 0, C.byref(h)) == capi.ERR_UNSUPPORTED
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=2)
    cfm.init(ds)
    assert L.nfm_cd_create(cfm._push(ds.ctx), 1e-6, 1e-3, 1e-3, 0, 1.0, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert L.nfm_gcd_create(cfm._push(ds.ctx), 1e-6, 1e-3, 1e-5, 0, 1.0, 100, 1e-7, 0, C.byref(h)) == 0
    try:
        ds.set_targets(np.ascontiguousarray(y, dtype=np.float64))
        rec = (C.c_double * 8)()
        ls, vs = C.c_double(0.0), C.c_double(0.0)
        assert L.nfm_opt_epoch(h, ds.h, None, 0, X.n, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
        assert L.nfm_hazan_iter(h, ds.h, 0, (C.c_double * X.d)(*([1.0] * X.d)), rec) == capi.ERR_INVALID
        assert L.nfm_gcd_outer_begin(h, ds.h, rec) == capi.ERR_INVALID  # before begin_fit
        lo, ro = C.c_double(0.0), C.c_double(0.0)
        assert L.nfm_gcd_begin_fit(h, ds.h, C.byref(lo), C.byref(ro)) == 0
        assert L.nfm_gcd_inner(h, ds.h, None, 0, rec) == capi.ERR_INVALID  # before outer_begin
        assert L.nfm_gcd_outer_begin(h, ds.h, rec) == 0
        assert L.nfm_gcd_inner(h, ds.h, None, 0, rec) == capi.ERR_INVALID  # a base is due: the start vector is missing
    finally:
        L.nfm_opt_destroy(h)
    # the command line keeps refusing --solver gcd and says where the solver is
    train = tmp_path / "train.svm"
    Xd = X.dense()
    with open(train, "w") as f:
        for i in range(X.n):
            f.write("%r %s\n" % (float(y[i]), " ".join("%d:%r" % (j + 1, float(Xd[i, j])) for j in range(X.d) if Xd[i, j] != 0.0)))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-m", "nimfm_amd", "train", "-t", "r", "--train", str(train), "--solver", "gcd"], capture_output=True,
                         text=True, env=env, timeout=300)
    assert out.returncode != 0 and "newGreedyCD" in out.stderr and "nimfm_cfm" in out.stderr and "dsyev" not in out.stderr
