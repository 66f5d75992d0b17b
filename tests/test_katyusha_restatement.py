"""CPU: the plain-Python restatement of Katyusha (tests/katyusha_restatement.py) checked against a dense twin, the
quirk-ordered finalize against its closed form, and the conditions the fixed inputs of tests/katyusha_cases.py must meet so
that the GPU suite (tests/test_gpu_katyusha.py) cannot pass without reaching the interesting paths.

The reference ships no test for this solver.  The twin is tests/test_pgd_restatement.py's: the ANOVA kernel summed over all
index subsets in torch float64, autograd through it times the reference's own dloss -- for the snapshot's gradient over all
rows and for updateGradient over the rows of a mini-batch --, the sort-based prox and reg.eval written out in Python.
Tolerance: the reference's checkAlmostEqual defaults, rtol 1e-6 and atol 1e-9.

The GPU suite's tolerance is MBPSGD's (rtol 1e-9 / atol 1e-12, 1e-10 relative on the per-epoch scalars).  The bound asserted
here: on every fixed input the restatement's own spread (seq against pair sums, pivot against slow prox; max |dP| / max |P|,
|dw|, |db|) is at most 1e-11, a hundredth of it, and the zero patterns of the variants agree.  Katyusha's parameters depend
on the sums written in the restatement only through viol and lossVal, so seq against pair moves no parameter at all; pivot
against slow moves them by at most a few 1e-16."""
import numpy as np
import pytest

import katyusha_cases as Cs
import katyusha_restatement as K
import pgd_restatement as R
from common import assert_close, init_fm, make_fm_dataset
from test_pgd_restatement import TWIN, Twin


@pytest.fixture(scope="module")
def runs():
    return {name: Cs.restate(name)[1] for name in Cs.CASES}


def test_spread_of_the_restatement_is_a_hundredth_of_the_device_bound(runs):
    for name, r in runs.items():
        for kw in (dict(sums="pair"), dict(prox="slow"), dict(sums="pair", prox="slow")):
            q = Cs.restate(name, **kw)[1]
            spread = max(np.abs(r.P - q.P).max() / np.abs(r.P).max(), np.abs(r.w - q.w).max(), abs(r.b - q.b))
            print("spread %-24s %-28s %.3e" % (name, kw, spread))
            assert spread <= 1e-11, (name, kw, spread)
            assert np.array_equal(r.P == 0.0, q.P == 0.0), (name, kw)
            assert len(r.iters) == len(q.iters), (name, kw)
            for a, b in zip(r.iters, q.iters):
                assert abs(a["viol"] - b["viol"]) <= 1e-11 * abs(a["viol"]) and abs(a["lossVal"] - b["lossVal"]) <= 1e-11 * abs(a["lossVal"])


def test_inputs_keep_the_gpu_suite_honest(runs):
    shares = {name: float((r.P == 0.0).mean()) for name, r in runs.items()}
    assert any(0.25 < s < 1.0 for s in shares.values()), shares  # the prox zeroes more than a quarter of P and fewer than all
    # a stream wrap inside a mini-batch: n is no multiple of B and the epoch's stream is longer than n
    Xo, *_ , stream = Cs.inputs("grid_l1")
    B = Cs.CASES["grid_l1"]["B"]
    assert Xo.n % B != 0 and runs["grid_l1"].inner * B > Xo.n and (Xo.n // B) * B < Xo.n < (Xo.n // B + 1) * B
    assert runs["converges"].converged and len(runs["converges"].iters) < Cs.CASES["converges"]["max_iter"]
    # delta is not small after one epoch from a random start: a gradient taken at one parameter set only cannot pass
    assert any(len(r.iters) > 1 and r.iters[1]["delta_ratio"] >= 1e-3 for r in runs.values())
    assert runs["grid_l1"].iters[1]["delta_ratio"] >= 1e-3
    s = Cs.inputs("sample_twice")[-1]
    assert s[0] == s[1]
    assert runs["one_inner"].inner == 1 and runs["batch_one"].batch == 1 and runs["many_features"].inner == 2
    assert runs["tau1_derived"].tau1 == runs["tau1_derived"].tau2 == 1.0 / 16.0 and runs["tau2_given"].tau2 == 0.2


def test_finalize_is_the_quirk_ordered_combination(runs):
    r = runs["grid_sql12"]
    m, t1, t2 = float(r.inner), r.tau1, r.tau2
    den = t1 * t2 + 1 - m - t1
    want = (t1 * t2 * r.tilde.P + (1 - m - t1) * r.y.P) / den
    np.testing.assert_allclose(r.P, want.transpose(0, 2, 1), rtol=1e-13, atol=0)
    np.testing.assert_allclose(r.w, (t1 * t2 * r.tilde.w + (1 - m - t1) * r.y.w) / den, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(r.b, (t1 * t2 * r.tilde.b + (1 - m - t1) * r.y.b) / den, rtol=1e-13, atol=0)
    assert abs((t1 * t2 + (1 - m - t1)) / den - 1.0) < 1e-15  # an affine combination, not the intended convex one
    # without fitLinear / fitIntercept finalize leaves the model's w / intercept alone
    q = runs["flags_squared_neither"]
    Xo, y, P0, w0, b0, n_aug, _ = Cs.inputs("flags_squared_neither")
    assert np.array_equal(q.w, w0) and q.b == b0


# ---------------------------------------------------------------- the dense twin
class KTwin(K.Katyusha):
    """every oracle-built piece replaced by a definition (tests/test_pgd_restatement.py's Twin)"""
    _model, predict, eval = Twin._model, Twin.predict, Twin.eval

    def __init__(self, Xd, *a, **kw):
        super().__init__(*a, prox="slow", **kw)
        import torch
        self.torch = torch
        self.Xd_all = torch.tensor(Xd, dtype=torch.float64)
        self.Xd = self.Xd_all

    def _grad_rows(self, p, rows):
        t = self.torch
        self.Xd = self.Xd_all[t.tensor(np.asarray(rows, dtype=np.int64))]
        try:
            P, w, b = (t.tensor(v, dtype=t.float64, requires_grad=True) for v in (p.P, p.w, p.b))
            yp = self._model(P, w, b)
            dl = R.loss_fns(self.loss, self.loss_param)[1]
            dL = np.array([dl(yi, pi) for yi, pi in zip(self.y[rows].tolist(), yp.detach().numpy().tolist())])
            yp.backward(t.tensor(dL / float(len(rows))))
            g = R.Params(P.grad.numpy(), w.grad.numpy() if self.fl else np.zeros_like(p.w), float(b.grad) if self.fi else 0.0)
            return yp.detach().numpy(), g
        finally:
            self.Xd = self.Xd_all

    def grad(self, p):
        return self._grad_rows(p, np.arange(self.n))

    def batch_grad(self, p, rows):
        return self._grad_rows(p, rows)[1]


@pytest.mark.parametrize("reg,transpose,degree", TWIN)
def test_restatement_matches_the_dense_twin(reg, transpose, degree):
    n, d, k, B = 30, 5, 3, 8
    losses = [("squared", "regression"), ("huber", "regression"), ("squared_hinge", "classification"), ("logistic", "classification")]
    flags = [(True, True), (False, True), (True, False), (False, False)]
    for q, ((loss, task), (fl, fi)) in enumerate(zip(losses, flags)):  # every loss and every flag pair, (False, True) included
        fit_lower = ("explicit", "augment", "none", "explicit")[q]
        Xo, Xd, y = make_fm_dataset(n, d, degree, k, 7 + q, fit_lower, fl, fi, threshold=0.3)
        P0, w0, b0, n_aug = init_fm(d, degree, k, fit_lower, fl, seed=2, scale=0.3)
        b0 = 0.1 if fi else 0.0
        kw = dict(reg=reg, transpose=transpose, loss=loss, task=task, gamma=1e-2, alpha0=1e-3, alpha=1e-2, beta=1e-2, batch=B, eta=0.05,
                  tau1=(0.5, -1.0)[q % 2], tau2=(-1.0, 0.2)[q // 2])
        stream = Cs.stream_of(n, 3 * 32, 5, twice=(q == 1))
        a = K.Katyusha(Xo, y, degree, n_aug, fl, fi, **kw).fit(P0, w0, b0, stream, max_iter=3, tol=0.0)
        b = KTwin(Xd, Xo, y, degree, n_aug, fl, fi, **kw).fit(P0, w0, b0, stream, max_iter=3, tol=0.0)
        tag = "%s deg %d %s lin %s icpt %s" % (reg, degree, loss, fl, fi)
        assert_close(a.P, b.P, what=tag + " P")
        assert_close(a.w, b.w, what=tag + " w")
        assert_close(a.b, b.b, what=tag + " b")
        for key in ("viol", "lossVal", "regVal"):
            assert_close([i[key] for i in a.iters], [i[key] for i in b.iters], what=tag + " " + key)


def test_refusals():
    Xo, _, y = make_fm_dataset(10, 4, 3, 2, 1)
    for reg in ("squaredl12", "squaredl21"):
        with pytest.raises(ValueError):
            K.Katyusha(Xo, y, 3, 0, True, True, reg=reg)
    with pytest.raises(ValueError):
        K.Katyusha(Xo, y, 2, 0, True, True, reg="omegati")
