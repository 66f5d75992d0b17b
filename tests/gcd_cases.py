"""Fixed inputs of the GreedyCD tests (tests/test_gcd_restatement.py on the CPU, tests/test_gpu_gcd.py on the device), all
generated from seeds; the generators are hazan_cases'.

Conditioning decides what can be compared at all.  Greedy CD fits the residual away component by component, so a late
component's gradient matrix has a small eigengap and the power method amplifies rounding differences.  The inputs plant
factors of distinct scales with label noise 0.02 and run few outer iterations; tests/test_gcd_restatement.py guards every case
used on the device (tree sums against in-order sums at least 100x below the tolerance of the device comparison), and
DROP_P_ROWS names the cases whose last P rows are left out of the comparison instead."""
import itertools

import numpy as np

import hazan_cases as hc

# the reference's grid (tests/test_greedy_cd.nim:92-135)
GRID = dict(maxComponents=6, maxIter=10, maxIterInner=10, nRefitting=10, tol=0.0, tolPower=0.0, maxIterPower=1000, alpha0=1e-6, alpha=1e-3,
            beta=1e-5)
WIDE = dict(maxComponents=3, maxIter=3, maxIterInner=4, nRefitting=2, tol=0.0, tolPower=0.0, maxIterPower=100, alpha0=1e-6, alpha=1e-3,
            beta=1e-5)


def grid_flags():
    """ignoreDiag x fitLinear x fitIntercept"""
    return list(itertools.product([True, False], repeat=3))


def _labels(y):
    return np.where(y > np.median(y), 1.0, -1.0)


def case(name):
    """-> (Data, y, keyword arguments of gcd_fit)"""
    kind, _, rest = name.partition(":")
    if kind == "grid":  # grid:<ignoreDiag><fitLinear><fitIntercept> as 0/1
        ig, fl, fi = (c == "1" for c in rest)
        X, y = hc.grid_data(fl, fi)
        return X, y, dict(GRID, ignoreDiag=ig, fitLinear=fl, fitIntercept=fi)
    if kind == "loss":  # the other three losses, as classification, one flag combination each
        ig, fl, fi = LOSS_FLAGS[rest]
        X, y = hc.grid_data(fl, fi)
        return X, _labels(y), dict(GRID, **LOSS_PARAMS[rest], ignoreDiag=ig, fitLinear=fl, fitIntercept=fi, loss=rest, task="classification")
    if kind == "wide":  # wide:<ignoreDiag><fitLinear>[:logistic]
        flags, _, lossname = rest.partition(":")
        ig, fl = (c == "1" for c in flags)
        X, y = hc.wide_data()
        kw = dict(WIDE, ignoreDiag=ig, fitLinear=fl, fitIntercept=True)
        if lossname:
            return X, _labels(y), dict(kw, loss=lossname, task="classification")
        return X, y, kw
    if kind == "branch":
        X, y = hc.grid_data(True, True, scales=BRANCH_SCALES.get(rest, hc.SCALES))
        return X, y, dict(GRID, ignoreDiag=True, fitLinear=True, fitIntercept=True, **BRANCH[rest])
    raise KeyError(name)


LOSS_FLAGS = {"squared_hinge": (True, True, True), "logistic": (False, True, False), "huber": (True, False, True)}
LOSS_PARAMS = {"squared_hinge": dict(maxIter=4), "logistic": dict(maxIter=4), "huber": dict(maxIter=3)}

BRANCH = {
    # a large beta: a new component is thresholded to zero, stays stored, and its slot is the next one used
    "big_beta": dict(beta=0.08, maxIter=3, maxIterInner=5, nRefitting=2),
    # two slots: once both hold non-zero lams the inner iterations run no power method
    "full_basis": dict(maxComponents=2, maxIter=3, maxIterInner=4, nRefitting=2),
    # a refit after every inner iteration, under a beta that lets refitDiag drive a component to zero
    "refit1": dict(beta=0.02, maxIter=3, maxIterInner=5, nRefitting=1),
    # nRefitting > maxIterInner: refitDiag never runs
    "norefit": dict(maxIter=3, maxIterInner=4, nRefitting=5),
    # the three stops with margins on both sides
    "power_stop": dict(tolPower=1e-7, maxIterPower=1000, maxIter=2, maxIterInner=3, nRefitting=10, maxComponents=3),
    "tol_stop": dict(tol=2e-3, maxIter=10, maxIterInner=10, nRefitting=1, maxComponents=3),
}
BRANCH_SCALES = {"power_stop": hc.POWER_STOP_SCALES}

GRID_CASES = ["grid:%d%d%d" % f for f in grid_flags()]
LOSS_CASES = ["loss:squared_hinge", "loss:logistic", "loss:huber"]
WIDE_CASES = ["wide:11", "wide:01", "wide:10", "wide:11:logistic"]
BRANCH_CASES = ["branch:" + k for k in BRANCH]
DEVICE_CASES = GRID_CASES + LOSS_CASES + WIDE_CASES + BRANCH_CASES

# cases whose last rows of P (late components: a small eigengap) are left out of the device comparison; at most two rows, and
# never in the wide case.  lams, w and the intercept are always compared (the reference's own test compares only those).
DROP_P_ROWS = {}

# the device comparison's tolerances (tests/test_gpu_hazan.py's)
TOL = dict(P_rtol=1e-6, P_atol=1e-9, w_rtol=1e-6, w_atol=1e-9, lams_atol=1e-7, intercept_atol=1e-5, obj_rtol=1e-8)


def starts(count, d, seed=1):
    """the start vectors the host draws after randomize(seed), by draw index"""
    return hc.nim_starts(seed, count, d)
