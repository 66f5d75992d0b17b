"""Fixed inputs of the PSGD tests (tests/test_psgd_lazy_restatement.py on the CPU, tests/test_gpu_psgd_lazy.py on the device),
built from seeds with tests/common.py's generators.  Every case is (data, model, solver settings, explicit permutations);
its restatement (tests/psgd_lazy_restatement.py, L1 under l1_reset = "consistent") is computed once and shared."""
import functools
import itertools

import numpy as np

import common
import psgd_lazy_restatement as R

REGS = ("l1", "l21")


class Case:
    def __init__(self, name, X, y, *, degree=2, k=4, fit_lower="explicit", fit_linear=True, fit_intercept=True, task="regression",
                 epochs=5, seed=1, scale=0.01, shuffle=True, **solver):
        self.name, self.X, self.y = name, X, np.asarray(y, dtype=np.float64)
        self.model = dict(task=task, degree=degree, fit_lower=fit_lower, fit_linear=fit_linear, fit_intercept=fit_intercept)
        self.k, self.epochs = k, epochs
        self.n_aug = R.n_augments(degree, fit_lower, fit_linear)
        rng = np.random.default_rng(seed)  # fm.init: w = 0, P ~ N(0, scale^2), b = 0 (factorization_machine.nim:125-139)
        self.P0 = rng.standard_normal((R.n_orders(degree, fit_lower), k, X.d + self.n_aug)) * scale
        self.w0, self.b0 = np.zeros(X.d), 0.0
        self.perms = common.make_perms(X.n, epochs, seed=7) if shuffle else None
        self.solver = dict(maxIter=epochs, tol=0.0)
        self.solver.update(solver)

    def restate(self, reg, **over):
        kw = dict(self.model)
        kw.update(self.solver)
        kw.update(reg=reg, perms=self.perms)
        kw.update(over)
        X = self.X
        return R.psgd_fit(X.indptr, X.indices, X.data, X.n, X.d, self.y, self.P0, self.w0, self.b0, **kw)

    @functools.lru_cache(maxsize=None)
    def reference(self, reg):
        """the restatement's fit of this case (L1: the consistent reset); shared, never modified"""
        return self.restate(reg)

    def __repr__(self):
        return self.name


def _planted(n, d, degree, k, seed, fit_lower="explicit", fit_linear=True, fit_intercept=True, threshold=0.3, scale=1.0):
    X, _, y = common.make_fm_dataset(n, d, degree, k, seed, fit_lower, fit_linear, fit_intercept, scale=scale, threshold=threshold)
    return X, y


# ---- the reference's grid (tests/test_psgd_l1.nim:99-135): n = 80, d = 8, k = 4, entries below 0.3 zeroed, 5 epochs ----
N, D, K = 80, 8, 4


@functools.lru_cache(maxsize=None)
def grid_case(degree, fit_lower, fit_linear, fit_intercept, gamma=1e-3):
    X, y = _planted(N, D, degree, K, 42, fit_lower, fit_linear, fit_intercept)
    return Case("grid-deg%d-%s-lin%d-int%d" % (degree, fit_lower, fit_linear, fit_intercept), X, y, degree=degree, k=K,
                fit_lower=fit_lower, fit_linear=fit_linear, fit_intercept=fit_intercept, gamma=gamma)


GRID = list(itertools.product((2, 3, 4), ("explicit", "none", "augment"), (False, True), (False, True)))


def grid_cases():
    return [grid_case(*g) for g in GRID]


@functools.lru_cache(maxsize=None)
def _base(degree=2, k=K, n=N, d=D, task="regression", data_scale=1.0):
    """data_scale: the planted model's scale (tests/utils.nim:29-47; 1.0 there).  0.3 keeps eta0 = 0.05 ... 0.1 stable."""
    X, y = _planted(n, d, degree, k, 42, scale=data_scale)
    if task == "classification":
        y = np.where(y - np.median(y) > 0, 1.0, -1.0)
    return X, y


def _case(name, degree=2, k=K, n=N, d=D, task="regression", data_scale=1.0, **kw):
    X, y = _base(degree, k, n, d, task, data_scale)
    return Case(name, X, y, degree=degree, k=k, task=task, **kw)


# ---- sparse: gamma chosen so that the final P is partly zero (between 20 % and 80 % exact zeros) ----
# (measured with the restatement: 59 %, 31 % and 75 % zeros)
SPARSE = {
    ("sparse-deg3", "l1"): dict(degree=3, eta0=0.05, gamma=5e-4, data_scale=0.3),
    ("sparse-deg3", "l21"): dict(degree=3, eta0=0.05, gamma=1e-3, data_scale=0.3),
    ("sparse-deg2", "l1"): dict(degree=2, eta0=0.05, gamma=1e-3, data_scale=0.3),
}


@functools.lru_cache(maxsize=None)
def sparse_case(name, reg):
    return _case("%s-%s" % (name, reg), **SPARSE[(name, reg)])


def sparse_cases():
    return [(sparse_case(name, reg), reg) for (name, reg) in SPARSE]


# ---- the two dense events ----
@functools.lru_cache(maxsize=None)
def cache_reset_case():
    # beta = 2 shrinks every parameter by 5/6 per step: the scaling passes 1e-8 after 102 steps, and what is left of P is of
    # the order 1e-10 -- gamma must be far below that for P to end non-zero
    return _case("cache-reset", beta=2.0, eta0=0.1, scheduling="constant", epochs=2, gamma=1e-11)


@functools.lru_cache(maxsize=None)
def w_reset_case():
    return _case("w-reset", alpha=20.0, eta0=0.1, scheduling="constant", data_scale=0.3)  # scaling_w /= 3 per step: a reset every 19 steps


# ---- the other three losses, as classification; the other schedules ----
@functools.lru_cache(maxsize=None)
def loss_case(loss):
    return _case("loss-" + loss, task="classification", loss=loss)


LOSSES = ("squared_hinge", "logistic", "huber")

SCHEDULES = {
    "invscaling": dict(scheduling="invscaling"),
    "pegasos": dict(scheduling="pegasos", alpha0=1.0, alpha=1.0, beta=1.0),  # eta = 1 / (regul * it): the strengths set the first steps
    "power": dict(scheduling="optimal", power=0.75),
}


@functools.lru_cache(maxsize=None)
def schedule_case(name):
    return _case("schedule-" + name, **SCHEDULES[name])


# ---- widths: below a wavefront, exactly one, one more, two ----
WIDTHS = (3, 64, 65, 128)


@functools.lru_cache(maxsize=None)
def width_case(k):
    return _case("width-%d" % k, k=k, n=24, epochs=2, gamma=1e-3)


# ---- row lengths: an empty row, a one-entry row, a row with unsorted ids ----
@functools.lru_cache(maxsize=None)
def row_case(kind):
    import oracle as O
    X, y = _base(n=24)
    Xd = X.dense()
    if kind == "empty":
        Xd[5] = 0.0
    elif kind == "one":
        Xd[5] = 0.0
        Xd[5, 3] = 0.7
    X2 = O.Dataset.from_dense(Xd)
    if kind == "unsorted":
        lo, hi = int(X2.indptr[5]), int(X2.indptr[6])
        assert hi - lo >= 3
        idx, val = X2.indices.copy(), X2.data.copy()
        idx[lo:hi], val[lo:hi] = idx[lo:hi][::-1].copy(), val[lo:hi][::-1].copy()
        X2 = O.Dataset(X2.indptr, idx, val, X2.n, X2.d)
    return Case("row-" + kind, X2, y, k=K, epochs=2, gamma=1e-3, fit_lower="augment", degree=3)


ROW_KINDS = ("empty", "one", "unsorted")


# ---- long rows: n = 6, d = 256, 200 entries per row, k = 64: the per-sample table leaves the LDS ----
@functools.lru_cache(maxsize=None)
def long_row_case():
    X = common.random_csr(6, 256, 200, seed=3)
    rng = np.random.default_rng(4)
    y = rng.standard_normal(6)
    return Case("long-rows", X, y, k=64, epochs=2, gamma=1e-3, scale=0.01)


def device_cases():
    """every (case, reg) the device is compared on"""
    out = [(c, reg) for c in grid_cases() for reg in REGS]
    out += sparse_cases()
    for reg in REGS:
        out += [(cache_reset_case(), reg), (w_reset_case(), reg)]
        out += [(loss_case(l), reg) for l in LOSSES]
        out += [(schedule_case(s), reg) for s in SCHEDULES]
        out += [(width_case(k), reg) for k in WIDTHS]
        out += [(row_case(r), reg) for r in ROW_KINDS]
        out += [(long_row_case(), reg)]
    return out
