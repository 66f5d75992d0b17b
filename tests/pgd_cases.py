"""The fixed inputs shared by tests/test_pgd_restatement.py (CPU) and tests/test_gpu_pgd.py: small planted-model datasets
(tests/common.py) with injected parameters.  tests/test_pgd_restatement.py asserts on the restatement alone that these inputs
reach a line search of three trials, a FISTA restart, an NMAPGD V branch, a Barzilai-Borwein start other than 1, an exhausted
maxSearch budget and a fit that stops on viol < tol, and that every comparison made on them has a relative margin of at
least 1e-6."""
import numpy as np

from common import init_fm, make_fm_dataset
import pgd_restatement as R

N, D, K = 60, 10, 4

# name -> (algo, degree, fit_lower, fit_linear, fit_intercept, solver keywords, fit keywords)
CASES = {
    "pgd_l1": ("pgd", 2, "explicit", True, True, dict(reg="l1", gamma=1e-3), dict(max_iter=4, tol=0.0)),
    "pgd_sql12_deg2": ("pgd", 2, "explicit", True, True, dict(reg="squaredl12", gamma=1e-2), dict(max_iter=4, tol=0.0)),
    "pgd_budget": ("pgd", 3, "explicit", True, False, dict(reg="l21", gamma=1e-3, max_search=2), dict(max_iter=3, tol=0.0)),
    "pgd_converges": ("pgd", 2, "none", False, True, dict(reg="l1", gamma=1e-3, beta=1e-2), dict(max_iter=200, tol=1e-3)),
    "fista_l21": ("fista", 3, "explicit", True, True, dict(reg="l21", gamma=1e-3), dict(max_iter=8, tol=0.0)),
    "fista_restart": ("fista", 3, "explicit", True, True, dict(reg="l21", gamma=1e-3, max_search=2), dict(max_iter=6, tol=0.0)),
    "fista_sql21": ("fista", 2, "explicit", False, True, dict(reg="squaredl21", gamma=1e-2), dict(max_iter=8, tol=0.0)),
    "nmapgd_sql12": ("nmapgd", 2, "explicit", True, True, dict(reg="squaredl12", gamma=1e-3), dict(max_iter=8, tol=0.0)),
    "nmapgd_rowwise": ("nmapgd", 2, "explicit", True, True, dict(reg="squaredl12", transpose=False, gamma=1e-2), dict(max_iter=6, tol=0.0)),
    "nmapgd_l1_deg3": ("nmapgd", 3, "augment", True, True, dict(reg="l1", gamma=1e-3, sigma=0.5), dict(max_iter=8, tol=0.0)),
    "nmapgd_logistic": ("nmapgd", 2, "explicit", True, True, dict(reg="l1", gamma=1e-3, loss="logistic", task="classification"),
                        dict(max_iter=6, tol=0.0)),
}


def inputs(name, scale=0.3):
    algo, degree, fit_lower, fl, fi, skw, fkw = CASES[name]
    Xo, _, y = make_fm_dataset(N, D, degree, K, 42, fit_lower, fl, fi, threshold=0.3)
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, K, fit_lower, fl, seed=3, scale=scale)
    w0 = np.random.default_rng(8).uniform(-0.1, 0.1, Xo.d) if fl else w0
    b0 = 0.05 if fi else 0.0
    return Xo, y, P0, w0, b0, n_aug


def restate(name, sums="seq", prox="pivot", **fit_over):
    algo, degree, fit_lower, fl, fi, skw, fkw = CASES[name]
    Xo, y, P0, w0, b0, n_aug = inputs(name)
    s = R.Solver(algo, Xo, y, degree, n_aug, fl, fi, sums=sums, prox=prox, **skw)
    kw = dict(fkw)
    kw.update(fit_over)
    return s, s.fit(P0, w0, b0, **kw)
