"""Plain-Python restatement of the reference's full-batch proximal gradient solvers: optimizer/pgd.nim `linesearch` and `fit`
(:106-217), fista.nim `extrapolate` and `fit` (:46-141), nmapgd.nim (:49-268), with model/params.nim (`add`, `scale`, `step`,
`dot`, `<-`) and optimizer/utils.nim (`computeViol`, `regularization`, `objective`).  The gradient, the forward pass, the
matrix prox and reg.eval are the oracle's (oracle.fm_predict_all_with_grad, fm_decision_function, prox, reg_eval); the loops,
the steps and every reduction are written here.  numpy never fuses a multiply-add, so every product and sum is rounded as
in the reference's generated C.

Quirks kept (each is the reference's):
  * Params.add steps the intercept only when grad.fitLinear (params.nim:47); scale shrinks it whenever fitIntercept.
  * Params.dot gates w and the intercept on the flags; `<-` copies everything.
  * pgd.linesearch evaluates reg.eval(params.P[0]) once per order (pgd.nim:145-146); FISTA's accept test reads that value.
  * newNMAPGD stores alpha0: alpha (nmapgd.nim:44).  Its V branch sets regVal = v_loss (:244), which feeds c.
  * maxSearch <= 0 searches until the condition holds or eta < 1e-12.  viol < tol is on the SQUARED distance.
  * regularization squares norm(., 2), i.e. the rounded square root (utils.nim:56-59).
  * getStepSize is |ss / sr|, 1 when either sum is exactly 0; with fitIntercept and not fitLinear s keeps the intercept itself.

`sums` is the order of every reduction written here: "seq" (ascending, the reference's) or "pair" (a halving tree).  The
spread of the parameters between the two is the yardstick of the device tolerance (tests/test_pgd_restatement.py).
`prox` is "pivot" (the oracle's restatement of the reference's randomised pivoting) or "slow" (the exact sort-based operator).

fit() returns a Result: parameters in the model layout, per iteration {trials, eta, start, branch, lossVal, regVal, viol, t, c, q},
every comparison as (lhs, rhs), the verbose lines, and the optimizer state for a warm start."""
import math

import numpy as np

import oracle as O
from cd_restatement import loss_fns


def seq_sum_loop(a):
    acc = 0.0
    for v in np.asarray(a, dtype=np.float64).ravel().tolist():
        acc += v
    return acc


def seq_sum(a):
    """seq_sum_loop, vectorised: np.add.accumulate adds strictly left to right, one rounding per element, so the last
    running total is the loop's, bit for bit (tests/test_dense_grid_cases.py holds the two together).  A million elements
    take the loop 0.1 s, which the inputs of tests/dense_grid_cases.py cannot afford."""
    a = np.asarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    return 0.0 + float(np.add.accumulate(a)[-1])


def pair_sum(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    while a.size > 1:
        if a.size % 2:
            a = np.concatenate([a, [0.0]])
        a = a[0::2] + a[1::2]
    return float(a[0])


SUMS = {"seq": seq_sum, "pair": pair_sum}


class Params:
    """model/params.nim:5-10: P in the training layout [nOrders][d + nAug][k]"""

    def __init__(self, P, w, b):
        self.P, self.w, self.b = np.array(P, dtype=np.float64), np.array(w, dtype=np.float64), float(b)

    def copy(self):
        return Params(self.P, self.w, self.b)


def zeros_like(p):
    return Params(np.zeros_like(p.P), np.zeros_like(p.w), 0.0)


def prox_slow(reg, Pt, lam, transpose):
    """the exact operators: softthreshold / block shrink / the sort-based SquaredL12 vector operator"""
    Pt = np.array(Pt, dtype=np.float64)
    if reg == "l1":
        return np.sign(Pt) * np.maximum(np.abs(Pt) - lam, 0.0)
    if reg == "l21":
        out = np.zeros_like(Pt)
        for j in range(Pt.shape[0]):
            nrm = math.sqrt(seq_sum(Pt[j] * Pt[j]))
            if nrm > lam:
                out[j] = Pt[j] * (1.0 - lam / nrm)
        return out
    if reg == "squaredl12":
        if transpose:
            for s in range(Pt.shape[1]):
                Pt[:, s] = O.prox_squaredl12_slow(Pt[:, s], lam)
        else:
            for j in range(Pt.shape[0]):
                Pt[j] = O.prox_squaredl12_slow(Pt[j], lam)
        return Pt
    if reg == "squaredl21":
        norms = np.array([math.sqrt(seq_sum(Pt[j] * Pt[j])) for j in range(Pt.shape[0])])
        new = O.prox_squaredl12_slow(norms, lam)
        for j in range(Pt.shape[0]):
            if norms[j] != 0:
                Pt[j] = Pt[j] / norms[j]
            Pt[j] = Pt[j] * new[j]
        return Pt
    raise ValueError(reg)


def reg_eval_py(reg, Pt, transpose, sm):
    if reg == "l1":
        return sm(np.abs(Pt))
    if reg == "l21":
        return sm([math.sqrt(sm(r * r)) for r in Pt])
    if reg == "squaredl12":
        A = np.abs(Pt).T if transpose else np.abs(Pt)
        return sm([sm(r) ** 2 for r in A])
    if reg == "squaredl21":
        return sm([math.sqrt(sm(r * r)) for r in Pt]) ** 2
    raise ValueError(reg)


class Result:
    pass


class Solver:
    def __init__(self, algo, X, y, degree, n_aug, fit_linear, fit_intercept, reg="squaredl12", transpose=None, loss="squared",
                 loss_param=1.0, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, rho=0.5, sigma=None, eta=0.5, max_search=-1,
                 task="regression", sums="seq", prox="pivot"):
        if reg not in ("l1", "l21", "squaredl12", "squaredl21"):
            raise ValueError("no matrix prox for %r" % (reg,))
        if reg in ("squaredl12", "squaredl21") and degree != 2:  # initSGD, squaredl12.nim:103-105
            raise ValueError("%s supports only degree=2." % reg)
        if not 0.0 < rho < 1.0:
            raise ValueError("rho must lie in (0, 1)")
        self.algo, self.X, self.degree, self.n_aug = algo, X, degree, n_aug
        self.y = np.sign(np.asarray(y, dtype=np.float64)) if task == "classification" else np.asarray(y, dtype=np.float64)
        self.fl, self.fi = bool(fit_linear), bool(fit_intercept)
        self.reg = reg
        self.transpose = (reg == "squaredl12") if transpose is None else bool(transpose)
        self.loss, self.loss_param = loss, loss_param
        self.lossf = loss_fns(loss, loss_param)[0]
        self.alpha0 = alpha if algo == "nmapgd" else alpha0  # nmapgd.nim:44
        self.alpha, self.beta, self.gamma, self.rho = alpha, beta, gamma, rho
        self.sigma = (0.01 if algo == "nmapgd" else 1.0) if sigma is None else sigma
        self.eta_nm, self.max_search = eta, max_search
        self.sm, self.sums, self.prox_kind = SUMS[sums], sums, prox
        self.n = X.n
        self.margins = []
        # carried on the optimizer between warm-started fits
        self.t, self.c, self.q = 0.0, -1.0, 1.0
        self.z = self.old_y = self.old_x = self.old_y_grads = None

    # ---- model/params.nim ----
    def step(self, old, g, eta):
        P = (old.P + -eta * g.P) * (1.0 / (1.0 + eta * self.beta))
        w = (old.w + -eta * g.w) * (1.0 / (1.0 + eta * self.alpha)) if self.fl else old.w.copy()
        b = old.b
        if self.fi and self.fl:
            b += -eta * g.b
        if self.fi:
            b *= 1.0 / (1.0 + eta * self.alpha0)
        return Params(P, w, b)

    def add(self, dst, src, coef):
        dst.P = dst.P + coef * src.P
        if self.fl:
            dst.w = dst.w + coef * src.w
        if self.fi and self.fl:
            dst.b += coef * src.b

    def scale(self, dst, s):
        dst.P = dst.P * s
        if self.fl:
            dst.w = dst.w * s
        if self.fi:
            dst.b *= s

    def dot(self, a, b):
        r = self.sm(a.P * b.P)
        if self.fl:
            r += self.sm(a.w * b.w)
        if self.fi:
            r += a.b * b.b
        return r

    def viol(self, a, b):  # utils.computeViol
        r = self.sm((a.P - b.P) ** 2)
        if self.fl:
            r += self.sm((a.w - b.w) ** 2)
        if self.fi:
            r += (a.b - b.b) ** 2
        return r

    def regularization(self, p):  # utils.nim:56-59
        r = 0.5 * self.alpha0 * (p.b * p.b) + 0.5 * self.alpha * math.sqrt(self.sm(p.w * p.w)) ** 2
        r += 0.5 * self.beta * math.sqrt(self.sm(p.P * p.P)) ** 2
        return r

    def eval(self, Pt):
        if self.sums == "seq":
            return O.reg_eval(self.reg, Pt, self.transpose)
        return reg_eval_py(self.reg, Pt, self.transpose, self.sm)

    def prox(self, p, lam):
        for o in range(p.P.shape[0]):
            if self.prox_kind == "slow":
                p.P[o] = prox_slow(self.reg, p.P[o], lam, self.transpose)
            else:
                p.P[o] = O.prox(self.reg, p.P[o], lam, self.transpose)

    # ---- pgd.nim:54-103 ----
    def model_P(self, p):
        return np.ascontiguousarray(p.P.transpose(0, 2, 1))

    def predict(self, p):
        return O.fm_decision_function(self.X, self.degree, self.model_P(p), p.w, p.b, self.n_aug)

    def grad(self, p):
        yp, _, gP, gw, gb = O.fm_predict_all_with_grad(self.X, self.y, self.degree, self.model_P(p), p.w, p.b, self.loss, self.n_aug,
                                                       self.fl, self.fi, self.loss_param)
        return yp, Params(gP, gw, gb)

    def mean_loss(self, yp):
        return self.sm([self.lossf(a, b) for a, b in zip(self.y.tolist(), np.asarray(yp).tolist())]) / float(self.n)

    def le(self, lhs, rhs):
        self.margins.append((lhs, rhs))
        return lhs <= rhs

    def gt(self, lhs, rhs):
        self.margins.append((lhs, rhs))
        return lhs > rhs

    # ---- pgd.nim:106-146 ----
    def linesearch_pgd(self, old, g, yp):
        eta, it, trials = 1.0, 0, 0
        old_loss = self.mean_loss(yp)
        dot_old = self.dot(old, g)
        while it < self.max_search or self.max_search <= 0:
            p = self.step(old, g, eta)
            self.prox(p, self.gamma * eta / (1.0 + eta * self.beta))
            lossVal = self.mean_loss(self.predict(p))
            trials += 1
            cond = self.dot(p, g) - dot_old
            cond += 0.5 * self.viol(p, old) / eta
            if self.le(lossVal - old_loss, self.sigma * cond) or eta < 1e-12:
                break
            eta *= self.rho
            it += 1
        regVal = self.regularization(p)
        for _ in range(p.P.shape[0]):
            regVal += self.gamma * self.eval(p.P[0])  # always order 0 (pgd.nim:146)
        return p, lossVal, regVal, eta, trials

    # ---- nmapgd.nim:102-130 ----
    def linesearch_nm(self, old, g, eta0, c):
        eta, it, trials = eta0, 0, 0
        while it < self.max_search or self.max_search <= 0:
            p = self.step(old, g, eta)
            self.prox(p, self.gamma * eta / (1.0 + eta * self.beta))
            lossVal = self.mean_loss(self.predict(p))
            regVal = self.regularization(p)
            for o in range(p.P.shape[0]):
                regVal += self.gamma * self.eval(p.P[o])
            trials += 1
            cond = self.viol(p, old)
            if self.le(lossVal + regVal - c, -self.sigma * cond) or eta < 1e-12:
                break
            eta *= self.rho
            it += 1
        return p, lossVal, regVal, cond, eta, trials

    def step_size(self, a, b, g, h):  # nmapgd.nim:89-99
        s, r = a.copy(), g.copy()
        self.add(s, b, -1.0)
        self.add(r, h, -1.0)
        ss, sr = self.dot(s, s), self.dot(s, r)
        return 1.0 if ss == 0.0 or sr == 0.0 else abs(ss / sr)

    def objective_full(self, p, lossVal):
        r = self.regularization(p)
        for o in range(p.P.shape[0]):
            r += self.gamma * self.eval(p.P[o])
        return lossVal + r

    def fit(self, P0, w0, b0, max_iter=100, tol=None, warm_start=False, callback=None, verbose=0):
        tol = (1e-5 if self.algo == "nmapgd" else 1e-6) if tol is None else tol
        x = Params(np.asarray(P0, dtype=np.float64).transpose(0, 2, 1), w0, b0)
        iters, lines = [], []
        if verbose > 0:
            lines.append("%s   %s   %s   Regularization" % ("Epoch".ljust(len(str(max_iter))), "Violation".ljust(10), "Loss".ljust(10)))
        self.margins = []
        converged = False
        if self.algo == "fista":
            old, z = x.copy(), x.copy()
            if not warm_start:
                self.t = 0.0
            lossAcc, regAcc = math.inf, math.inf
        elif self.algo == "nmapgd":
            if not warm_start:
                self.t, self.c, self.q = 0.0, -1.0, 1.0
            if self.t == 0.0 or self.z is None or self.z.P.shape != x.P.shape:
                self.z, self.old_y_grads = zeros_like(x), zeros_like(x)
                self.old_y, self.old_x = x.copy(), x.copy()
            if self.c < 0:
                self.c = self.objective_full(x, self.mean_loss(self.predict(x)))
        for it in range(max_iter):
            rec = {"trials": (0, 0), "eta": (0.0, 0.0), "start": (1.0, 0.0), "branch": "none"}
            if self.algo == "pgd":
                old = x.copy()
                yp, g = self.grad(x)
                x, lossVal, regVal, eta, trials = self.linesearch_pgd(old, g, yp)
                rec.update(trials=(trials, 0), eta=(eta, 0.0))
                viol = self.viol(x, old)
            elif self.algo == "fista":
                t = (math.sqrt(4 * (self.t * self.t) + 1.0) + 1.0) / 2.0
                coef = (self.t - 1) / t
                z = x.copy()
                self.add(z, x, coef)
                self.add(z, old, -coef)
                old = z.copy()
                yp, g = self.grad(z)
                z, z_loss, z_reg, eta, trials = self.linesearch_pgd(old, g, yp)
                rec.update(trials=(trials, 0), eta=(eta, 0.0))
                if self.le(z_loss + z_reg, lossAcc + regAcc):
                    lossAcc, regAcc = z_loss, z_reg
                    old = x.copy()
                    x = z.copy()
                    self.t = t
                    rec["branch"] = "accept"
                else:
                    self.t = 1.0
                    rec["branch"] = "restart"
                lossVal, regVal = lossAcc, regAcc
                viol = self.viol(x, old)
            else:
                t = (math.sqrt(4 * (self.t * self.t) + 1.0) + 1.0) / 2.0
                y_ = self.z.copy()
                self.scale(y_, self.t / t)
                self.add(y_, x, (t - 1) / t)
                self.add(y_, self.old_x, -(self.t - 1) / t)
                self.old_x = x.copy()
                yp, yg = self.grad(y_)
                step_z = self.step_size(y_, self.old_y, yg, self.old_y_grads)
                cz = self.objective_full(y_, self.mean_loss(yp))
                self.z, z_loss, z_reg, cond, eta_z, tr_z = self.linesearch_nm(y_, yg, step_z, max(cz, self.c))
                v_loss = v_reg = math.inf
                eta_v, tr_v, step_v = 0.0, 0, 0.0
                if self.gt(z_loss + z_reg, self.c - self.sigma * cond):
                    _, xg = self.grad(x)
                    step_v = self.step_size(x, self.old_y, xg, self.old_y_grads)
                    x, v_loss, v_reg, _, eta_v, tr_v = self.linesearch_nm(self.old_x, xg, step_v, self.c)
                    rec["step_v"] = step_v
                if self.le(z_loss + z_reg, v_loss + v_reg):
                    lossVal, regVal = z_loss, z_reg
                    x = self.z.copy()
                    rec["branch"] = "z"
                else:
                    lossVal, regVal = v_loss, v_loss  # nmapgd.nim:244
                    rec["branch"] = "v"
                self.old_y, self.old_y_grads = y_.copy(), yg.copy()
                self.t = t
                self.c = self.eta_nm * self.c * self.q + lossVal + regVal
                self.q = self.eta_nm * self.q + 1
                self.c /= self.q
                rec.update(trials=(tr_z, tr_v), eta=(eta_z, eta_v), step_z=step_z, start=(step_z, step_v))
                viol = self.viol(x, self.old_x)
            rec.update(lossVal=lossVal, regVal=regVal, viol=viol, t=self.t, c=self.c, q=self.q)
            iters.append(rec)
            if callback is not None:
                callback(self.model_P(x), x.w.copy(), x.b)
            if verbose > 0:
                lines.append("%s   %-10.4e   %-10.4e   %-10.4e" % (str(it + 1).ljust(max(5, len(str(max_iter)))), viol, lossVal, regVal))
            if viol < tol:
                if verbose > 0:
                    lines.append("Converged at epoch %d." % (it if self.algo == "pgd" else it + 1))
                converged = True
                break
        if not converged and verbose > 0:
            lines.append("Objective did not converge. Increase maxIter.")
        r = Result()
        r.P, r.w, r.b = self.model_P(x), x.w.copy(), x.b
        r.iters, r.lines, r.margins, r.converged = iters, lines, list(self.margins), converged
        return r
