"""Plain-Python restatement of the reference's Katyusha: optimizer/katyusha.nim `finalize` (:56-73), `epoch` (:76-153) and
`fit` (:156-269), with nmapgd.extrapolate (nmapgd.nim:133-138), minibatch_psgd.updateGradient (:67-88) and the Params helpers
of tests/pgd_restatement.py (`add`, `scale`, `step`, `<-`, computeViol, regularization).  The gradients, the matrix prox and
reg.eval are the oracle's (oracle.fm_predict_all_with_grad -- on the rows of a mini-batch, in the stream's order, for
updateGradient, and on all rows for the snapshot --, oracle.prox, oracle.reg_eval); the loops, the steps and every reduction
are written here.  numpy never fuses a multiply-add.

The gradient of one inner iteration is formed as  grads = grads_ave + (g(params) - g(tilde))  with each g the mini-batch's
sum in sample order times 1 / miniBatchSize: the association the device uses.  The reference adds the samples' two
contributions to grads_ave one after the other (katyusha.nim:105-112); the two differ by rounding only, far below the
tolerance of tests/test_gpu_katyusha.py (the spread test of tests/test_katyusha_restatement.py bounds what summation
order can move).

Quirks kept (each is the reference's):
  * Params.add steps w only when fitLinear and the intercept only when fitIntercept and fitLinear (params.nim:41-48); scale
    gates on the flags; `<-` copies everything.  With fitIntercept and not fitLinear the intercept only decays and
    next_tilde's intercept stays 0, so tilde's is 0 after the first epoch.
  * fit calls finalize(sfm, tilde, y, float(maxIterInner), tau1, tau2) on a proc declared (..., tau1, tau2, m): the model is
    (tau1 tau2 tilde + (1 - m - tau1) y) / (tau1 tau2 + 1 - m - tau1); the division is element-wise (tensor.nim:453-455).
  * lossVal is the loss at the snapshot the epoch started from; regVal is taken on tilde.
  * nothing is carried between fits.

`sums` and `prox` are pgd_restatement's switches.  fit() returns a Result: the finalized model in the model layout, per
epoch {viol, lossVal, regVal, delta_ratio}, the verbose lines, tilde, and whether the fit converged."""
import math

import numpy as np

import oracle as O
import pgd_restatement as R
from pgd_restatement import Params, Result, zeros_like


class Katyusha(R.Solver):
    def __init__(self, X, y, degree, n_aug, fit_linear, fit_intercept, eta=0.1, batch=-1, tau1=0.5, tau2=-1.0, **kw):
        super().__init__("katyusha", X, y, degree, n_aug, fit_linear, fit_intercept, **kw)
        self.eta, self.batch, self.tau1_arg, self.tau2_arg = eta, batch, tau1, tau2

    # ---- minibatch_psgd.nim:67-88 over the rows of one mini-batch: (1 / B) sum_i dloss_i dA_i in the stream's order ----
    def batch_grad(self, p, rows):
        X = self.X
        lens = (X.indptr[1:] - X.indptr[:-1])[rows]
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = np.concatenate([np.arange(X.indptr[i], X.indptr[i + 1]) for i in rows]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
        Xs = O.Dataset(indptr, X.indices[take], X.data[take], len(rows), X.d)
        _, _, gP, gw, gb = O.fm_predict_all_with_grad(Xs, self.y[rows], self.degree, self.model_P(p), p.w, p.b, self.loss, self.n_aug,
                                                      self.fl, self.fi, self.loss_param)
        return Params(gP, gw, gb)

    # ---- katyusha.nim:56-73 as fit calls it (:238, :269) ----
    def finalize(self, tilde, y, inner, tau1, tau2, w0, b0):
        f_tau1, f_tau2, f_m = float(inner), tau1, tau2  # the proc's own names for what fit passes
        den = f_tau2 * f_m + 1.0 - f_tau1 - f_tau2
        P = f_m * f_tau2 * tilde.P
        P = P + (1 - f_tau1 - f_tau2) * y.P
        P = P / den
        w, b = np.array(w0, dtype=np.float64), float(b0)
        if self.fl:
            w = f_m * f_tau2 * tilde.w
            w = w + (1 - f_tau1 - f_tau2) * y.w
            w = w / den
        if self.fi:
            b = f_m * f_tau2 * tilde.b
            b += (1 - f_tau1 - f_tau2) * y.b
            b /= den
        return np.ascontiguousarray(P.transpose(0, 2, 1)), w, b

    # ---- katyusha.nim:76-153 ----
    def epoch(self, z, y, tilde, gave, stream, ii, B, inner, tau1, tau2):
        m = float(inner)
        th = [1.0 + min(self.eta * s, 1.0 / (4.0 * m)) for s in (self.beta, self.alpha, self.alpha0)]  # P, w, intercept
        pw = [1.0, 1.0, 1.0]
        nt = zeros_like(tilde)
        tau3 = 1 - tau1 - tau2
        ratio = 0.0
        for _ in range(inner):
            x = z.copy()  # nmapgd.extrapolate
            self.scale(x, tau1)
            self.add(x, tilde, tau2)
            self.add(x, y, tau3)
            rows = np.asarray(stream[ii:ii + B], dtype=np.int64)
            assert len(rows) == B, "the index stream is too short"
            ii += B
            gx, gt = self.batch_grad(x, rows), self.batch_grad(tilde, rows)
            g = gave.copy()
            dP = gx.P - gt.P
            g.P = gave.P + dP
            if self.fl:
                g.w = gave.w + (gx.w - gt.w)
            if self.fi:
                g.b = gave.b + (gx.b - gt.b)
            ratio = max(ratio, float(np.abs(dP).max()) / max(float(np.abs(gave.P).max()), 1e-300))
            z = self.step(z, g, self.eta)
            self.prox(z, self.gamma * self.eta / (1.0 + self.beta * self.eta))
            self.scale(y, tau3)
            self.add(y, tilde, tau2)
            self.add(y, z, tau1)
            nt.P = nt.P + pw[0] * y.P  # Params.add with one coefficient per part
            if self.fl:
                nt.w = nt.w + pw[1] * y.w
            if self.fi and self.fl:
                nt.b += pw[2] * y.b
            pw = [a * b for a, b in zip(pw, th)]
        coef = [(1.0 - t) / (1.0 - p) for t, p in zip(th, pw)]
        nt.P = nt.P * coef[0]
        if self.fl:
            nt.w = nt.w * coef[1]
        if self.fi:
            nt.b *= coef[2]
        return nt, z, y, ii, ratio

    # ---- katyusha.nim:156-269 ----
    def fit(self, P0, w0, b0, stream, max_iter=100, tol=1e-6, callback=None, verbose=0):
        n = self.n
        x = Params(np.asarray(P0, dtype=np.float64).transpose(0, 2, 1), w0, b0)
        y, z, tilde = x.copy(), x.copy(), x.copy()
        B = self.batch
        if B <= 0:
            B = max((self.X.d * n) // int(self.X.indptr[-1]), 1)
        inner = (n - 1) // B + 1
        tau2 = 1.0 / (2.0 * float(B)) if self.tau2_arg < 0 else self.tau2_arg
        tau1 = tau2 if self.tau1_arg < 0 else self.tau1_arg
        yp, gave = self.grad(tilde)
        iters, lines = [], []
        if verbose > 0:
            lines.append("Minibatch size: %d" % B)
            lines.append("Number of inner iteration: %d" % inner)
            lines.append("%s   %s   %s   Regularization" % ("Epoch".ljust(len(str(max_iter))), "Violation".ljust(10), "Loss".ljust(10)))
        converged, ii = False, 0
        for it in range(max_iter):
            nt, z, y, ii, ratio = self.epoch(z, y, tilde, gave, stream, ii, B, inner, tau1, tau2)
            viol = self.viol(nt, tilde)
            tilde = nt.copy()
            if callback is not None:
                callback(*self.finalize(tilde, y, inner, tau1, tau2, w0, b0))
            lossVal = self.mean_loss(yp)
            if math.isnan(lossVal):
                lines.append("Loss is NaN. Use smaller learning rate.")
                break
            regVal = self.regularization(tilde)
            for o in range(tilde.P.shape[0]):
                regVal += self.gamma * self.eval(tilde.P[o])
            iters.append(dict(viol=viol, lossVal=lossVal, regVal=regVal, delta_ratio=ratio))
            if verbose > 0:
                lines.append("%s   %-10.4e   %-10.4e   %-10.4e" % (str(it + 1).ljust(max(5, len(str(max_iter)))), viol, lossVal, regVal))
            if viol < tol:
                if verbose > 0:
                    lines.append("Converged at epoch %d." % (it + 1))
                converged = True
                break
            yp, gave = self.grad(tilde)
        if not converged and verbose > 0:
            lines.append("Objective did not converge. Increase maxIter.")
        r = Result()
        r.P, r.w, r.b = self.finalize(tilde, y, inner, tau1, tau2, w0, b0)
        r.tilde, r.y, r.z = tilde, y, z
        r.iters, r.lines, r.converged = iters, lines, converged
        r.batch, r.inner, r.tau1, r.tau2 = B, inner, tau1, tau2
        return r
