"""CPU: the plain-Python restatement of PGD, FISTA and NMAPGD (tests/pgd_restatement.py) checked against a dense twin, and
the conditions the fixed inputs of tests/pgd_cases.py must meet so that the GPU suite cannot pass without reaching the
interesting paths.

The reference ships no test for these solvers.  The twin replaces every piece the restatement takes from the oracle by one
built from a definition: the model is the ANOVA kernel summed over all index subsets in torch float64, the gradient comes
from autograd through the model (times the reference's own dloss), the prox is the exact sort-based operator (oracle.prox_squaredl12_slow) and reg.eval is written out in
Python.  The fit loops themselves (the line searches and the accept / restart and Z / V branches) are the restatement's:
what is independent is the arithmetic of every step, not the control flow.  Tolerance: the reference's own checkAlmostEqual
defaults, rtol 1e-6 and atol 1e-9.

Spread of the parameters between the restatement's sequential and pairwise runs (max |dP| / max |P|, |dw|, |db|), measured
on the fixed inputs: 0 for every PGD and FISTA input (their parameters depend on the sums only through decisions, and no
decision changes); nmapgd_sql12 3.3e-12, nmapgd_rowwise 2.9e-15, nmapgd_l1_deg3 4.1e-15, nmapgd_logistic 8.9e-16 (the
Barzilai-Borwein start is a ratio of two sums).  All are below a tenth of the device tolerances (1e-10, and 1e-9 where the
deterministic threshold stands in for pivoting), so tests/test_gpu_pgd.py uses those tolerances unwidened.  The bound below
re-measures it."""
import itertools
import math

import numpy as np
import pytest

import oracle as O
import pgd_cases as Cs
import pgd_restatement as R
from common import assert_close, init_fm, make_fm_dataset


def rel_margin(a, b):
    m = max(abs(a), abs(b))
    return 1.0 if not (math.isfinite(a) and math.isfinite(b)) or m == 0.0 else abs(a - b) / m


@pytest.fixture(scope="module")
def runs():
    return {name: Cs.restate(name)[1] for name in Cs.CASES}


def test_inputs_reach_every_path(runs):
    its = [(n, i) for n, r in runs.items() for i in r.iters]
    assert any(max(i["trials"]) >= 3 for _, i in its), "no line search of three trials"
    assert any(i["branch"] == "restart" for _, i in its), "no FISTA restart"
    assert any(i["branch"] == "v" for _, i in its), "no NMAPGD V branch"
    assert any("step_z" in i and i["step_z"] != 1.0 for _, i in its), "no Barzilai-Borwein start other than 1"
    budget = Cs.CASES["pgd_budget"][5]["max_search"]
    assert any(i["trials"][0] == budget and i["eta"][0] == 0.5 ** budget for i in runs["pgd_budget"].iters), "no exhausted budget"
    assert runs["pgd_converges"].converged and len(runs["pgd_converges"].iters) < Cs.CASES["pgd_converges"][6]["max_iter"]


def test_every_comparison_has_a_margin(runs):
    for name, r in runs.items():
        assert r.margins
        worst = min(rel_margin(a, b) for a, b in r.margins)
        assert worst >= 1e-6, (name, worst)


def test_summation_order_moves_no_decision_and_little_else(runs):
    for name, r in runs.items():
        r2 = Cs.restate(name, sums="pair")[1]
        assert [(i["trials"], i["branch"]) for i in r.iters] == [(i["trials"], i["branch"]) for i in r2.iters], name
        spread = max(np.abs(r.P - r2.P).max() / np.abs(r.P).max(), np.abs(r.w - r2.w).max(), abs(r.b - r2.b))
        print("spread %-18s %.3e" % (name, spread))
        assert spread <= 1e-11, (name, spread)  # a tenth of 1e-10


# ---------------------------------------------------------------- the dense twin
class Twin(R.Solver):
    """every oracle-built piece replaced by a definition (see the module docstring)"""

    def __init__(self, Xd, *a, **kw):
        super().__init__(*a, prox="slow", **kw)
        import torch
        self.torch = torch
        self.Xd = torch.tensor(Xd, dtype=torch.float64)

    def _model(self, P, w, b):  # P [O][da][k]
        t = self.torch
        n, d = self.Xd.shape
        Xa = t.cat([self.Xd, t.ones((n, self.n_aug), dtype=t.float64)], 1)
        out = self.Xd @ w + b
        for o in range(P.shape[0]):
            m = self.degree - o
            for idx in itertools.combinations(range(Xa.shape[1]), m):
                term = t.ones((n, P.shape[2]), dtype=t.float64)
                for j in idx:
                    term = term * (Xa[:, j:j + 1] * P[o, j][None, :])
                out = out + term.sum(1)
        return out

    def predict(self, p):
        t = self.torch
        return self._model(t.tensor(p.P), t.tensor(p.w), t.tensor(p.b, dtype=t.float64)).numpy()

    def grad(self, p):
        t = self.torch
        P, w, b = (t.tensor(v, dtype=t.float64, requires_grad=True) for v in (p.P, p.w, p.b))
        yp = self._model(P, w, b)
        # dloss is the reference's own (loss.nim, restated in tests/cd_restatement.py; its Huber derivative is kept as written),
        # the model's derivative is autograd's
        dl = R.loss_fns(self.loss, self.loss_param)[1]
        dL = np.array([dl(yi, pi) for yi, pi in zip(self.y.tolist(), yp.detach().numpy().tolist())])
        yp.backward(t.tensor(dL / float(self.n)))
        g = R.Params(P.grad.numpy(), w.grad.numpy() if self.fl else np.zeros_like(p.w), float(b.grad) if self.fi else 0.0)
        return yp.detach().numpy(), g

    def eval(self, Pt):
        return R.reg_eval_py(self.reg, Pt, self.transpose, R.seq_sum)


TWIN = [(reg, tr, deg) for reg, tr, degs in (("l1", False, (2, 3)), ("l21", False, (2, 3)), ("squaredl12", True, (2,)),
                                              ("squaredl12", False, (2,)), ("squaredl21", False, (2,))) for deg in degs]


@pytest.mark.parametrize("algo", ["pgd", "fista", "nmapgd"])
@pytest.mark.parametrize("reg,transpose,degree", TWIN)
def test_restatement_matches_the_dense_twin(algo, reg, transpose, degree):
    n, d, k = 30, 5, 3
    losses = [("squared", "regression"), ("huber", "regression"), ("squared_hinge", "classification"), ("logistic", "classification")]
    flags = [(True, True), (False, True), (True, False), (False, False)]
    for q, ((loss, task), (fl, fi)) in enumerate(zip(losses, flags)):  # every loss and every flag pair, (False, True) included
        fit_lower = ("explicit", "augment", "none", "explicit")[q]
        Xo, Xd, y = make_fm_dataset(n, d, degree, k, 7 + q, fit_lower, fl, fi, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(d, degree, k, fit_lower, fl, seed=2, scale=0.3)
        b0 = 0.1 if fi else 0.0
        kw = dict(reg=reg, transpose=transpose, loss=loss, task=task, gamma=1e-2, alpha0=1e-3, alpha=1e-2, beta=1e-2)
        # NMAPGD with Huber: the reference's Huber derivative (loss.nim, kept) points uphill, every line search runs down to
        # eta < 1e-12 and leaves the point unchanged to ~1e-12, and the next Barzilai-Borwein start is then a ratio of two sums of
        # such differences -- measured 34.04 against 34.16 between the two gradient implementations.  That ratio is ill-posed
        # for ANY input, so this one combination is compared over its first iteration (start 1) only.
        iters = 1 if (algo == "nmapgd" and loss == "huber") else 4
        a = R.Solver(algo, Xo, y, degree, n_aug, fl, fi, **kw).fit(P0, w0, b0, max_iter=iters, tol=0.0)
        b = Twin(Xd, algo, Xo, y, degree, n_aug, fl, fi, **kw).fit(P0, w0, b0, max_iter=iters, tol=0.0)
        tag = "%s %s deg %d %s lin %s icpt %s" % (algo, reg, degree, loss, fl, fi)
        assert [(i["trials"], i["branch"]) for i in a.iters] == [(i["trials"], i["branch"]) for i in b.iters], tag
        assert_close(a.P, b.P, what=tag + " P")
        assert_close(a.w, b.w, what=tag + " w")
        assert_close(a.b, b.b, what=tag + " b")
        assert_close([i["viol"] for i in a.iters], [i["viol"] for i in b.iters], what=tag + " viol")


def test_refusals():
    Xo, _, y = make_fm_dataset(10, 4, 3, 2, 1)
    for reg in ("squaredl12", "squaredl21"):
        with pytest.raises(ValueError):
            R.Solver("pgd", Xo, y, 3, 0, True, True, reg=reg)
    with pytest.raises(ValueError):
        R.Solver("pgd", Xo, y, 2, 0, True, True, reg="omegati")
    with pytest.raises(ValueError):
        R.Solver("pgd", Xo, y, 2, 0, True, True, reg="l1", rho=1.0)


def test_warm_start_keeps_the_state():
    s, r = Cs.restate("nmapgd_sql12", max_iter=3)
    t, c, q = s.t, s.c, s.q
    assert t > 1.0 and q > 1.0 and c >= 0.0
    r2 = s.fit(r.P, r.w, r.b, max_iter=1, tol=0.0, warm_start=True)
    whole = Cs.restate("nmapgd_sql12", max_iter=4)[1]
    np.testing.assert_array_equal(r2.P, whole.P)  # 3 + 1 warm-started iterations are the 4 of one fit
