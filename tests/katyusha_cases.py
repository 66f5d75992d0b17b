"""The fixed inputs shared by tests/test_katyusha_restatement.py (CPU) and tests/test_gpu_katyusha.py: small datasets with
injected parameters and an explicit index stream (concatenated permutations, so the stream wraps where the reference's
`ii mod nSamples == 0` would reshuffle).  tests/test_katyusha_restatement.py asserts on the restatement alone the conditions
that keep the GPU suite honest: the restatement's own spread is at most 1e-11 on every input, the prox zeroes a share of P
on one, a wrap falls inside a mini-batch on one, one converges early and delta is not small on one."""
import numpy as np

import oracle as O
from common import init_fm, make_fm_dataset, random_csr
import dense_grid_cases as G
import katyusha_restatement as K


def stream_of(n, need, seed, twice=False):
    rng = np.random.default_rng(seed)
    out = []
    while sum(len(a) for a in out) < need:
        out.append(rng.permutation(n))
    s = np.concatenate(out)[:need].astype(np.int64)
    if twice:  # the same sample twice in the first mini-batch
        s[1] = s[0]
    return s


def _planted(n, d, k, degree, fit_lower, fl, fi, seed=5, scale=0.3, loss="squared", zero_rows=False):
    Xo, _, y = make_fm_dataset(n, d, degree, k, seed, fit_lower, fl, fi, threshold=0.3)
    if loss in ("logistic", "squared_hinge"):
        y = np.sign(y)
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fl, seed=3, scale=scale)
    w0 = np.random.default_rng(8).uniform(-0.1, 0.1, Xo.d) if fl else w0
    if zero_rows:  # every other feature starts at zero: where the penalty outweighs the gradient it stays there, in every set
        P0[:, :, ::2] = 0.0
    return Xo, y, P0, w0, (0.05 if fi else 0.0), n_aug


def _random(n, d, m, k, scale=0.3):
    Xo = random_csr(n, d, m, 3)
    y = np.random.default_rng(4).normal(size=n)
    P0, w0, b0, n_aug = init_fm(d, 2, k, "explicit", True, scale=scale)
    return Xo, y, P0, w0, 0.0, n_aug


def _heavy():
    n, d = 1200, 3000
    rng = np.random.default_rng(8)
    Xo = random_csr(n, 12, 5, 1)  # 12 hot features ...
    idx = Xo.indices.reshape(n, 5).copy()
    idx[:, 4] = rng.integers(12, d, size=n)  # ... and one cold one per row
    Xo = O.Dataset(Xo.indptr, idx.reshape(-1), Xo.data, n, d)
    y = rng.normal(size=n)
    P0, w0, b0, n_aug = init_fm(d, 2, 8, "explicit", True, scale=0.2)
    return Xo, y, P0, w0, 0.0, n_aug


def _many_features():
    n, d = 32, 20000
    Xo = random_csr(n, d, 40, 6)
    y = np.random.default_rng(2).normal(size=n)
    P0, w0, b0, n_aug = init_fm(d, 2, 2, "explicit", True, scale=0.3)
    return Xo, y, P0, w0, 0.0, n_aug


def _case(data, degree=2, fit_lower="explicit", fl=True, fi=True, task="regression", B=16, max_iter=3, tol=0.0, twice=False, **skw):
    return dict(data=data, degree=degree, fit_lower=fit_lower, fl=fl, fi=fi, task=task, B=B, max_iter=max_iter, tol=tol, twice=twice, skw=skw)


def _grid(reg, degree, fit_lower, gamma, zero_rows=False):
    return _case(lambda: _planted(83, 9, 4, degree, fit_lower, True, True, zero_rows=zero_rows), degree, fit_lower, reg=reg, gamma=gamma)


def _flags(loss, fl, fi):
    task = "regression" if loss in ("squared", "huber") else "classification"
    return _case(lambda: _planted(64, 8, 3, 2, "explicit", fl, fi, loss=loss), fl=fl, fi=fi, task=task, B=8, max_iter=2, reg="squaredl12",
                 gamma=1e-2, loss=loss, eta=0.05)


def _padded(reg, transpose, k):
    return _case(lambda: _random(60, 40, 6, k), B=12, max_iter=2, reg=reg, transpose=transpose, gamma=0.05)


CASES = {
    # MBPSGD's grid: n = 83, d = 9, k = 4, B = 16 -- six inner iterations, 96 positions per epoch: the stream wraps inside a batch
    "grid_l1": _grid("l1", 2, "explicit", 0.2, zero_rows=True),
    "grid_l21": _grid("l21", 2, "explicit", 0.2, zero_rows=True),
    "grid_sql12": _grid("squaredl12", 2, "explicit", 0.2, zero_rows=True),
    "grid_sql21": _grid("squaredl21", 2, "explicit", 0.2, zero_rows=True),
    "grid_l1_deg3": _grid("l1", 3, "explicit", 0.02),
    "grid_l21_deg3_aug": _grid("l21", 3, "augment", 0.02),
    "grid_l1_deg4_none": _grid("l1", 4, "none", 0.02),
    "grid_l1_aug": _grid("l1", 2, "augment", 0.05),
    # the flag / loss combinations of MBPSGD's test_flags_losses_schedules
    "flags_logistic": _flags("logistic", True, True),
    "flags_sqhinge_nolinear": _flags("squared_hinge", False, True),  # fitIntercept without fitLinear: the intercept quirk
    "flags_huber_nointercept": _flags("huber", True, False),
    "flags_squared_neither": _flags("squared", False, False),
    # padded and wide rows
    "pad_sql12_col_k5": _padded("squaredl12", True, 5),
    "pad_sql12_row_k5": _padded("squaredl12", False, 5),
    "pad_l21_k17": _padded("l21", None, 17),
    "pad_sql21_k33": _padded("squaredl21", False, 33),
    "pad_sql12_row_k33": _padded("squaredl12", False, 33),
    "pad_sql12_col_k17": _padded("squaredl12", True, 17),
    # the schedule's corners
    "one_inner": _case(lambda: _planted(40, 8, 3, 2, "explicit", True, True), B=64, max_iter=3, reg="l1", gamma=0.02),  # B >= n: m = 1
    "batch_one": _case(lambda: _planted(12, 6, 3, 2, "explicit", True, True), B=1, max_iter=2, reg="l21", gamma=0.02),
    "tau1_derived": _case(lambda: _planted(40, 8, 3, 2, "explicit", True, True), B=8, max_iter=2, reg="l1", gamma=0.02, tau1=-1.0),
    "tau2_given": _case(lambda: _planted(40, 8, 3, 2, "explicit", True, True), B=8, max_iter=2, reg="squaredl12", gamma=0.02, tau2=0.2, tau1=0.3),
    "sample_twice": _case(lambda: _planted(40, 8, 3, 2, "explicit", True, True), B=8, max_iter=2, reg="l1", gamma=0.02, twice=True),
    "heavy": _case(_heavy, B=600, max_iter=2, reg="squaredl12", gamma=0.01),
    "many_features": _case(_many_features, B=16, max_iter=1, reg="squaredl12", gamma=1e-2),  # d > 16384, 2 inner iterations
    "converges": _case(lambda: _planted(40, 8, 3, 2, "none", False, True), fit_lower="none", fl=False, B=8, max_iter=60, tol=1e-3, reg="l1",
                       gamma=0.05, beta=1e-2),
}

# The large-grid inputs of tests/dense_grid_cases.py: two or three inner iterations, one or two epochs.  Their CPU conditions
# (spread, share of zeros, delta not small) are stated in tests/test_dense_grid_cases.py, case by case, so that
# tests/test_katyusha_restatement.py keeps walking the small inputs above only.
def _large(shape, B, max_iter, **skw):
    return _case(lambda: G.data(shape, 0.3, zero_rows=True), B=B, max_iter=max_iter, **skw)


# gamma: the prox zeroes between 5 % and 95 % of z where P0 is not zero, and (all but tall_sql21, whose threshold outweighs every
# gradient step) some of the touched rows that start at zero leave it and some stay: the final zero pattern is the prox's doing
GRID_CASES = {
    "tall_l1": _large("tall", 16, 2, reg="l1", gamma=0.03),  # most features are never stamped: their rows follow grads_ave alone
    "tall_sql21": _large("tall", 24, 2, reg="squaredl21", gamma=3e-6),
    "deep_l21": _large("deep", 24, 2, reg="l21", gamma=1.5),
    "deep_sql12_col": _large("deep", 16, 1, reg="squaredl12", gamma=1e-4),  # the STEP and REST split over three trips
    "passes_sql12_col": _large("passes", 32, 1, reg="squaredl12", gamma=5e-5),
    # the first Katyusha fit of a model with more than 128 factors (kc = 2)
    "wide_l1_k130": _case(lambda: _random(60, 40, 6, 130), B=12, max_iter=2, reg="l1", gamma=0.05),
}


def case(name):
    return CASES[name] if name in CASES else GRID_CASES[name]


def inputs(name):
    c = case(name)
    Xo, y, P0, w0, b0, n_aug = c["data"]()
    inner = (Xo.n - 1) // c["B"] + 1
    stream = stream_of(Xo.n, c["max_iter"] * c["B"] * inner, 11, c["twice"])
    return Xo, y, P0, w0, b0, n_aug, stream


def restate(name, sums="seq", prox="pivot", **fit_over):
    c = case(name)
    Xo, y, P0, w0, b0, n_aug, stream = inputs(name)
    s = K.Katyusha(Xo, y, c["degree"], n_aug, c["fl"], c["fi"], batch=c["B"], task=c["task"], sums=sums, prox=prox, **c["skw"])
    kw = dict(max_iter=c["max_iter"], tol=c["tol"])
    kw.update(fit_over)
    return s, s.fit(P0, w0, b0, stream, **kw)
