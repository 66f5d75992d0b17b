"""tests/gcd_restatement.py held to the brute force of the reference's own test, the branches the device cases must reach, and
the conditioning guard of tests/test_gpu_gcd.py.  No GPU."""
import functools

import numpy as np
import pytest

import gcd_cases as gc
import gcd_restatement as gr
import hazan_cases as hc


@functools.lru_cache(maxsize=None)
def fits(name):
    """(in-order sums, the device's trees forced to the same discrete decisions) of one case, computed once"""
    X, y, kw = gc.case(name)
    st = gc.starts(64, X.d)
    a = gr.gcd_fit(X, y, st, summation="order", **kw)
    b = gr.gcd_fit(X, y, st, summation="tree", forced=gr.counts_of(a.history), **kw)
    return a, b


def inner_records(res):
    return [r for o in res.history for r in o["inner"]]


# ---- 1. the restatement against the brute force, on the reference's grid (tests/test_greedy_cd.nim:92-135) ----
@pytest.mark.parametrize("ignoreDiag,fitLinear,fitIntercept", gc.grid_flags())
def test_restatement_matches_brute_force(ignoreDiag, fitLinear, fitIntercept):
    X, y = hc.grid_data(fitLinear, fitIntercept)
    assert (X.n, X.d) == (50, 6)
    st = gc.starts(64, X.d)
    kw = dict(maxComponents=6, ignoreDiag=ignoreDiag, fitLinear=fitLinear, fitIntercept=fitIntercept, maxIter=10, alpha0=1e-6, alpha=1e-3,
              beta=1e-5, maxIterInner=10, nRefitting=10, maxIterPower=1000)
    fast = gr.gcd_fit(X, y, st, tol=0.0, tolPower=0.0, **kw)
    slow = gr.brute_force_fit(X.dense(), y, st, **kw)
    lams = np.zeros(6)
    lams[:len(fast.lams)] = fast.lams
    print("d intercept %.3e  d w %.3e  d lams %.3e" % (abs(fast.intercept - slow.intercept), np.abs(fast.w - slow.w).max(),
                                                    np.abs(lams - slow.lams).max()))
    assert abs(fast.intercept - slow.intercept) < 1e-5  # :132
    assert np.all(np.abs(fast.w - slow.w) <= 1e-5 + 1e-6 * np.abs(slow.w))  # :133
    assert np.all(np.abs(lams - slow.lams) <= 1e-9 + 1e-5 * np.abs(slow.lams))  # :134
    if not fitLinear:
        assert np.all(fast.w == 0.0)
    if not fitIntercept:
        assert fast.intercept == 0.0


# ---- 2. the device cases reach the branches they are there for ----
def test_branch_new_component_thresholded_and_slot_reused():
    for name in ("branch:big_beta", "branch:refit1"):
        recs = inner_records(fits(name)[0])
        hits = [k for k, r in enumerate(recs) if r["slot"] >= 0 and not r["added"]]
        assert hits, name  # a base whose lams the soft threshold set to zero: stored, not counted
        k = hits[0]
        assert recs[k]["lam"] == 0.0 and recs[k]["nStored"] > recs[k]["nComponents"]
        nxt = next(r for r in recs[k + 1:] if r["slot"] >= 0)
        assert nxt["slot"] == recs[k]["slot"] and nxt["nStored"] == recs[k]["nStored"]  # re-used, not appended


def test_branch_full_basis_runs_no_power_method():
    a = fits("branch:full_basis")[0]
    recs = inner_records(a)
    assert any(r["slot"] >= 0 for r in recs) and any(r["slot"] < 0 and r["powerIters"] == 0 for r in recs)
    assert len(a.lams) == 2 and a.draws == 2


def test_branch_refit_drives_a_component_to_zero():
    for name in ("branch:big_beta", "branch:refit1"):
        a = fits(name)[0]
        hit = False
        for o in a.history:
            before = o["nComponentsStart"]
            for r in o["inner"]:
                if r["refit"] and r["nComponents"] < before + r["added"]:
                    hit = True
                before = r["nComponents"]
        assert hit, name


def test_branch_no_refit():
    X, y, kw = gc.case("branch:norefit")
    assert kw["nRefitting"] > kw["maxIterInner"]
    recs = inner_records(fits("branch:norefit")[0])
    assert recs and not any(r["refit"] for r in recs)
    assert all(r["checked"] == (bool(r["added"]) or r["it"] == kw["maxIterInner"] - 1) for r in recs)


def test_branch_warm_start_begins_with_components():
    X, y, kw = gc.case("grid:111")
    st = gc.starts(64, X.d)
    one = gr.gcd_fit(X, y, st, **dict(kw, maxIter=1))
    assert len(one.lams) > 0
    two = gr.gcd_fit(X, y, lambda k, d: st(one.draws + k, d), warm=one, **dict(kw, maxIter=1))
    assert two.history[0]["nComponentsStart"] == int(np.count_nonzero(one.lams)) > 0
    assert two.loss0 == pytest.approx(one.history[-1]["loss"], rel=1e-12)


def test_branch_stops_fire_with_margins():
    a = fits("branch:power_stop")[0]
    X, y, kw = gc.case("branch:power_stop")
    runs = [r for r in inner_records(a) if r["slot"] >= 0]
    assert runs and all(1 < r["powerIters"] < kw["maxIterPower"] for r in runs)  # the power stop, not the cap
    lo, hi = 1 - 1e-3, 1 + 1e-3  # the margin on both sides of a threshold: the guard below measures rounding at 1e-13 relative
    for r in runs:
        assert r["powerDiff"] < kw["tolPower"] * lo and r["powerDiffPrev"] > kw["tolPower"] * hi
    a = fits("branch:tol_stop")[0]
    X, y, kw = gc.case("branch:tol_stop")
    assert a.converged and len(a.history) < kw["maxIter"]  # the outer stop
    assert any(len(o["inner"]) < kw["maxIterInner"] for o in a.history)  # the inner stop
    for o in a.history:
        last = o["inner"][-1]
        if len(o["inner"]) < kw["maxIterInner"]:
            assert last["innerDiff"] < kw["tol"] * lo
        for r in o["inner"][:-1]:
            assert not r["checked"] or r["innerDiff"] > kw["tol"] * hi
    assert a.history[-1]["outerDiff"] < kw["tol"] * lo and all(o["outerDiff"] > kw["tol"] * hi for o in a.history[:-1])


def test_tree_and_order_take_the_same_decisions():
    """without forcing: the stops and the thresholds fall the same way under the device's summation"""
    for name in gc.BRANCH_CASES:
        X, y, kw = gc.case(name)
        a = fits(name)[0]
        t = gr.gcd_fit(X, y, gc.starts(64, X.d), summation="tree", **kw)
        assert gr.counts_of(a.history) == gr.counts_of(t.history), name
        assert [(r["slot"], r["added"], r["nComponents"]) for r in inner_records(a)] == [(r["slot"], r["added"], r["nComponents"])
                                                                                          for r in inner_records(t)], name


# ---- 3. the conditioning guard: the device's trees against in-order sums, 100x below the device comparison's tolerances ----
@pytest.mark.parametrize("name", gc.DEVICE_CASES)
def test_conditioning_guard(name):
    a, b = fits(name)
    T = gc.TOL
    keep = a.P.shape[0] - gc.DROP_P_ROWS.get(name, 0)
    assert gc.DROP_P_ROWS.get(name, 0) <= 2 and not (name.startswith("wide") and name in gc.DROP_P_ROWS)
    assert a.P.shape == b.P.shape and [(r["slot"], r["added"]) for r in inner_records(a)] == [(r["slot"], r["added"]) for r in inner_records(b)]
    rP = (np.abs(a.P - b.P) / (T["P_atol"] + T["P_rtol"] * np.abs(a.P)))[:keep].max() if keep else 0.0
    rw = (np.abs(a.w - b.w) / (T["w_atol"] + T["w_rtol"] * np.abs(a.w))).max()
    rl = np.abs(a.lams - b.lams).max() / T["lams_atol"] if len(a.lams) else 0.0
    rb = abs(a.intercept - b.intercept) / T["intercept_atol"]
    oa = np.array([r["objective"] for r in inner_records(a)] + [o["loss"] + o["reg"] for o in a.history])
    ob = np.array([r["objective"] for r in inner_records(b)] + [o["loss"] + o["reg"] for o in b.history])
    ro = (np.abs(oa - ob) / np.abs(oa)).max() / T["obj_rtol"]
    print("%s: fraction of the tolerance  P %.2e  w %.2e  lams %.2e  intercept %.2e  objectives %.2e" % (name, rP, rw, rl, rb, ro))
    assert max(rP, rw, rl, rb, ro) <= 1e-2
