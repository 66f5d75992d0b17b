"""The restatement of Hazan's algorithm (tests/hazan_restatement.py) and the convex model's text format, on the CPU.

  - the restatement against a brute-force dense Hazan that follows the reference's tests/optimizer/hazan_slow.nim, on the
    reference's grid and at the reference's tolerances (tests/test_hazan.nim);
  - the conditioning guard: on every case the device tests use, tree sums against in-order sums move P, lams, w and every
    record's loss by less than 1e-8 relative -- 1/100 of the parity tolerance;
  - the branches the cases must reach;
  - dump / load of the reference's text format."""
import numpy as np
import pytest

import hazan_cases as hc
import hazan_restatement as hr


def _kw(shape, optimal, ignoreDiag, fitLinear, fitIntercept, **over):
    kw = dict(maxComponents=shape["maxComponents"], ignoreDiag=ignoreDiag, fitLinear=fitLinear, fitIntercept=fitIntercept,
              maxIter=shape["maxIter"], eta=shape["eta"], tol=shape["tol"], maxIterPower=shape["maxIterPower"],
              tolPower=shape["tolPower"], optimal=optimal)
    kw.update(over)
    return kw


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300)) if a.size else 0.0


_RUNS = {}


def _grid_run(flags):
    """the in-order restatement of a grid case, computed once and shared (never modified)"""
    if flags not in _RUNS:
        optimal, ignoreDiag, fitLinear, fitIntercept = flags
        X, y = hc.grid_data(fitLinear, fitIntercept)
        kw = _kw(hc.GRID, *flags)
        _RUNS[flags] = (X, y, kw, hr.hazan_fit(X, y, hc.nim_starts(1, kw["maxIter"], X.d), **kw))
    return _RUNS[flags]


@pytest.fixture(scope="module")
def wide_runs():
    X, y = hc.wide_data()
    out = {}
    for ignoreDiag, optimal, fitLinear, fitIntercept in hc.WIDE_RUNS:
        kw = _kw(hc.WIDE, optimal, ignoreDiag, fitLinear, fitIntercept)
        out[(ignoreDiag, optimal, fitLinear, fitIntercept)] = (kw, hr.hazan_fit(X, y, hc.numpy_starts(100), **kw))
    return X, y, out


@pytest.mark.parametrize("flags", hc.grid_flags())
def test_against_brute_force(flags):
    optimal, ignoreDiag, fitLinear, fitIntercept = flags
    X, y, kw, run = _grid_run(flags)
    brute = hr.brute_force_fit(X.dense(), y, hc.nim_starts(1, kw["maxIter"], X.d), maxComponents=kw["maxComponents"], ignoreDiag=ignoreDiag,
                               fitLinear=fitLinear, fitIntercept=fitIntercept, maxIter=kw["maxIter"], eta=kw["eta"],
                               maxIterPower=kw["maxIterPower"], optimal=optimal)
    np.testing.assert_allclose(run.P, brute.P, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(run.w, brute.w, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(run.lams, brute.lams, rtol=0.0, atol=1e-7)
    assert abs(run.intercept - brute.intercept) < 1e-5
    if not fitLinear:
        assert not run.w.any()
    if not fitIntercept:
        assert run.intercept == 0.0


def _guard(X, y, starts, kw, run):
    forced = [(r["powerIters"], r["cgIters"]) for r in run.history]
    tree = hr.hazan_fit(X, y, starts, summation="tree", forced=forced, **kw)
    worst = max(_rel(tree.P, run.P), _rel(tree.lams, run.lams), _rel(tree.w, run.w),
                max(abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(tree.history, run.history)))
    assert [a["slot"] for a in tree.history] == [b["slot"] for b in run.history]
    assert worst < 1e-8, worst


@pytest.mark.parametrize("flags", hc.grid_flags())
def test_conditioning_guard_grid(flags):
    X, y, kw, run = _grid_run(flags)
    _guard(X, y, hc.nim_starts(1, kw["maxIter"], X.d), kw, run)


@pytest.mark.parametrize("flags", hc.WIDE_RUNS)
def test_conditioning_guard_wide(wide_runs, flags):
    X, y, runs = wide_runs
    kw, run = runs[tuple(flags)]
    _guard(X, y, hc.numpy_starts(100), kw, run)


def test_conditioning_guard_other_device_cases():
    """the classification fit and the power-stop cases of tests/test_gpu_hazan.py"""
    X, y = hc.grid_data(True, True)
    yc = np.where(y > np.median(y), 3.0, -2.0)
    kw = _kw(hc.GRID, True, True, True, True, maxIter=4)
    starts = hc.nim_starts(1, 4, X.d)
    _guard(X, yc, starts, dict(kw, task="classification"), hr.hazan_fit(X, yc, starts, task="classification", **kw))
    margins = 0
    for optimal, ignoreDiag, fitLinear, fitIntercept in hc.POWER_STOP_FLAGS:
        X, y = hc.grid_data(fitLinear, fitIntercept, scales=hc.POWER_STOP_SCALES)
        kw = _kw(hc.GRID, optimal, ignoreDiag, fitLinear, fitIntercept, tolPower=1e-7, maxIter=3)
        run = hr.hazan_fit(X, y, hc.numpy_starts(300), **kw)
        _guard(X, y, hc.numpy_starts(300), kw, run)
        margins += sum(r["powerDiff"] < 1e-7 / 2 and r["powerDiffPrev"] > 2e-7 for r in run.history)
    assert margins >= 1  # the power-stop test needs a stop with a margin of 2x on both sides


def test_branch_coverage(wide_runs):
    runs = [_grid_run(f) for f in hc.grid_flags()]
    hists = [(kw, run.history) for _, _, kw, run in runs] + [(kw, run.history) for kw, run in wide_runs[2].values()]
    assert any(kw["optimal"] and sum(1e-10 < r["step"] < 1.0 for r in h) >= 2 for kw, h in hists)
    assert any(kw["optimal"] and any(r["step"] == 1e-10 for r in h) for kw, h in hists)
    assert any(kw["optimal"] and kw["maxIter"] > kw["maxComponents"] and len(h) == kw["maxIter"]
               and any(r["slot"] < i and r["nComponents"] == kw["maxComponents"] for i, r in enumerate(h) if i >= kw["maxComponents"])
               for kw, h in hists)
    assert any(not kw["optimal"] and len(h) == kw["maxComponents"] < kw["maxIter"] for kw, h in hists)
    assert any(max(r["cgIters"] for r in h) >= 10 for kw, h in hists)  # the CG stop is live in the wide case


def test_forced_counts_reproduce_the_plain_run():
    X, y, kw, run = _grid_run((True, True, True, True))
    forced = [(r["powerIters"], r["cgIters"]) for r in run.history]
    again = hr.hazan_fit(X, y, hc.nim_starts(1, kw["maxIter"], X.d), forced=forced, **kw)
    assert again.P.tobytes() == run.P.tobytes() and again.w.tobytes() == run.w.tobytes() and again.it == run.it == kw["maxIter"]


def test_tree_sum_is_a_sum():
    rng = np.random.default_rng(0)
    for n, blk in ((1, 32), (31, 32), (33, 32), (300, 32), (2500, 256), (40000, 32)):
        a = rng.normal(size=n)
        assert abs(hr.tree_sum(a, blk) - float(np.sum(a))) <= 1e-12 * float(np.sum(np.abs(a)))
    assert hr.tree_sum(np.zeros(0), 32) == 0.0 and hr.ordered_sum(np.zeros(0)) == 0.0


def test_dump_load_round_trip(tmp_path):
    import nimfm_amd as nf

    rng = np.random.default_rng(3)
    cfm = nf.newConvexFactorizationMachine("classification", maxComponents=5, fitIntercept=False, fitLinear=True, ignoreDiag=False)
    with pytest.raises(nf.NotFittedError):
        cfm.dump(str(tmp_path / "never.txt"))
    P, lams, w = rng.normal(size=(3, 4)), np.array([0.1, 1e-10, 2.5]), rng.normal(size=4)
    cfm.set_params(P, lams, w, -0.125)
    path = str(tmp_path / "cfm.txt")
    cfm.dump(path)
    lines = open(path).read().split("\n")
    # the reference's field order (convex_factorization_machine.nim:93-107)
    assert [l.split(":")[0] for l in lines[:8]] == ["task", "nFeatures", "degree", "nComponents", "maxComponents", "fitIntercept", "fitLinear", "lams"]
    assert lines[:7] == ["task: classification", "nFeatures: 4", "degree: 2", "nComponents: 3", "maxComponents: 5", "fitIntercept: false",
                         "fitLinear: true"]
    assert lines[9] == "P:" and lines[13] == "w:" and lines[15] == "intercept: -0.125" and lines[16] == ""
    back = nf.load(path, True, ignoreDiag=False)
    assert isinstance(back, nf.ConvexFactorizationMachine)
    assert (back.task, back.maxComponents, back.fitIntercept, back.fitLinear, back.ignoreDiag, back.warmStart) == ("classification", 5, False, True, False, True)
    assert back.P.tobytes() == P.tobytes() and back.lams.tobytes() == lams.tobytes() and back.w.tobytes() == w.tobytes()
    assert back.intercept == -0.125 and back.isInitialized and back.nComponents == 3
    assert nf.load(path, False).ignoreDiag is True  # the format does not store it: the argument's default
    # zero components are legal
    empty = nf.newConvexFactorizationMachine("regression", maxComponents=2)
    empty.set_params(np.zeros((0, 4)), np.zeros(0), w, 1.5)
    empty.dump(path)
    back = nf.load(path, False)
    assert back.nComponents == 0 and back.P.shape == (0, 4) and back.intercept == 1.5


def test_model_constructor_and_solver_refusals():
    import nimfm_amd as nf

    with pytest.raises(ValueError, match="maxComponents < 1."):
        nf.newConvexFactorizationMachine("regression", maxComponents=0)
    cfm = nf.newConvexFactorizationMachine("r")
    assert (cfm.maxComponents, cfm.fitIntercept, cfm.fitLinear, cfm.ignoreDiag, cfm.warmStart, cfm.nComponents) == (30, True, True, True, False, 0)
    opt = nf.newHazan()
    assert (opt.maxIter, opt.eta, opt.verbose, opt.tol, opt.nTol, opt.maxIterPower, opt.tolPower, opt.optimal, opt.it) == \
        (100, 1000.0, 2, 1e-7, 10, 1000, 1e-7, True, 0)
    with pytest.raises(ValueError, match="ConvexFactorizationMachine"):
        opt.fit(None, None, nf.newFactorizationMachine("r"))
    for make in (nf.newSGD, nf.newAdaGrad, nf.newCD, nf.newPCD, nf.newPBCD, nf.newMBPSGD, nf.newPGD, nf.newFISTA, nf.newNMAPGD, nf.newKatyusha):
        with pytest.raises(ValueError, match="ConvexFactorizationMachine"):
            make(verbose=0).fit(None, None, cfm)


def test_uniform_draws_continue_the_global_stream():
    import nimfm_amd as nf

    nf.randomize(1)
    a = nf.globalRand().rand(5)
    b = nf.globalRand().rand(3)
    one = nf.NimRand(1).rand(8)
    assert np.concatenate([a, b]).tobytes() == one.tobytes()
    assert ((one >= 0.0) & (one < 1.0)).all() and len(set(one)) == 8
    assert (nf.NimRand(1).rand(4, 2.0) == 2.0 * one[:4]).all()
