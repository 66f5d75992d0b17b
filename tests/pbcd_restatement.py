"""Plain-Python restatement of the reference's proximal block coordinate descent: optimizer/pbcd.nim `fit` (:212-329) with
`update` (:112-157), `epoch` (:160-209), `computeDerivative` (:49-58) and `precomputeAnova` (:61-77) at maxSearch = 0, and
the BCD hooks of its three regularisers: L1 (l1.nim:31-33), L21 (l21.nim:25-29) and SquaredL21 (squaredl21.nim:32-43,
90-101, transpose = false).  Python floats are IEEE doubles and Python never fuses a multiply-add, so every sum and product
is rounded as in the reference's generated C.

PBCD steps the whole row P[j, 0..k) of a feature at once.  beta and gamma are NOT scaled by nSamples (alpha0 and alpha are,
:226-227); with one order the table A is built once and carried from iteration to iteration, with several it is rebuilt per
order and iteration (:292-299); the synchronisation at degree >= 3 leaves A[degree] untouched (:203-206).  With
maxSearch = 0 the running `value` of L1 and L21 is read by nothing, so only SquaredL21 keeps state (norms and cache).

order="reference" walks the features in ascending j.  order="level" walks CD's level schedule, reversed inside each level:
right for L1 and L21, wrong for SquaredL21, whose prox reads the running sum of every row's norm.  order="run" walks the run
schedule: per run of sample-disjoint consecutive features, every gradient from the state before the
run, then the proximal chain in ascending j, then the synchronisations (here in reverse).  The loss is the reference's
running total; the intercept, the w sweep and the dummy features keep the reference's sums (the device sums the intercept,
the dummies and the loss with a fixed tree).

`last_resums` counts how often SquaredL21's re-sum branch (squaredl21.nim:37-38) was taken in the last fit.
"""
import math

import numpy as np

from cd_restatement import columns, levels, loss_fns, total  # noqa: F401
from pcd_restatement import runs, softthreshold

last_resums = 0


def norm2(v):
    """norm(v, 2) (tensor.nim:608-616): the ascending sum of squares, then the square root"""
    acc = 0.0
    for x in v:
        acc += abs(x) * abs(x)
    return math.sqrt(acc)


def norm1(v):
    acc = 0.0
    for x in v:
        acc += abs(x)
    return acc


class Reg:
    """one regulariser's BCD hooks: initBCD, computeCacheBCD, prox, updateCacheBCD"""

    def __init__(self, name, transpose=False, degree=2, nFeatures=0):
        self.name = name
        self.resums = 0
        if name == "squaredl12":  # nimfm_sparsefm.nim:118
            raise ValueError("PBCD cannot be used for squaredl12.")
        if name not in ("l1", "l21", "squaredl21"):
            raise ValueError(name)
        if name == "squaredl21":  # initBCD, squaredl21.nim:68-73
            if degree != 2:
                raise ValueError("SquaredL21 supports only degree=2.")
            if transpose:
                raise ValueError("transpose=true is not supported for BCD.")
        self.norms = [0.0] * nFeatures
        self.cache = 0.0

    @property
    def chained(self):
        return self.name == "squaredl21"

    def compute_cache(self, Po):  # computeCacheBCD, Po [d + nAug][k]
        if self.name != "squaredl21":
            return
        acc = 0.0
        for j in range(len(Po)):
            self.norms[j] = norm2(Po[j])
        for v in self.norms:
            acc += v
        self.cache = acc

    def prox(self, pj, lam, j):  # in place
        if self.name == "l1":
            for s in range(len(pj)):
                pj[s] = softthreshold(pj[s], lam)
            return
        if self.name == "l21":
            nrm = norm2(pj)
            if nrm > lam:
                f = 1.0 - lam / nrm
                for s in range(len(pj)):
                    pj[s] *= f
            else:
                for s in range(len(pj)):
                    pj[s] = 0.0
            return
        for s in range(len(pj)):
            pj[s] /= (1 + 2 * lam)
        nrm = norm2(pj)
        if self.cache < self.norms[j]:
            self.resums += 1
            acc = 0.0
            for v in self.norms:
                acc += v
            self.cache = acc
        lamScaled = 2.0 * lam / (1.0 + 2 * lam) * (self.cache - self.norms[j])
        if nrm > lamScaled:
            f = 1.0 - lamScaled / nrm
            for s in range(len(pj)):
                pj[s] *= f
        else:
            for s in range(len(pj)):
                pj[s] = 0.0

    def update_cache(self, pj, j):  # updateCacheBCD
        if self.name != "squaredl21":
            return
        self.cache -= self.norms[j]
        self.norms[j] = norm2(pj)
        self.cache += self.norms[j]


def fit(indptr, indices, data, y, P, w, intercept, degree, nAugments, fitLinear, fitIntercept, maxIter=100, alpha0=1e-6,
        alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", lossParam=1.0, tol=1e-3, task="regression", reg="squaredl21",
        transpose=False, order="reference", callback=None, sums="seq"):
    """-> (P, w, intercept, history, converged); P [nOrders][k][d + nAugments] (copied), history [(viol, mean loss)].
    sums="pair": the intercept's and the dummy features' sums over every sample with np.sum, and the iteration's loss summed
    afresh with it (the device's fixed trees), as tests/cd_restatement.py does"""
    global last_resums
    n = len(indptr) - 1
    P = np.array(P, dtype=np.float64, copy=True)
    nOrders, k, da = P.shape
    d = da - nAugments
    w = np.array(w, dtype=np.float64, copy=True)
    b = float(intercept)
    y = [float(v) for v in y]
    if task == "classification":
        y = [float((v > 0) - (v < 0)) for v in y]
    lo, dl, mu = loss_fns(loss, lossParam)
    cols = columns(indptr, indices, data, n, d)
    cols_aug = cols + [[(i, 1.0) for i in range(n)] for _ in range(nAugments)]
    nf = float(n)
    a0n, an = alpha0 * nf, alpha * nf  # :226-227; beta and gamma stay unscaled
    R = Reg(reg, transpose, degree, da)
    lv = levels(cols, n)
    level_order = sorted(range(d), key=lambda j: (lv[j], -j))
    if order == "reference":
        groups = [[j] for j in range(da)]
    elif order == "level":
        groups = [[j] for j in level_order] + [[j] for j in range(d, da)]
    elif order == "run":
        groups = runs(cols) + [[j] for j in range(d, da)]
    else:
        raise ValueError(order)
    w_order = list(range(d)) if order == "reference" else level_order  # the w sweep is CD's
    pair = sums == "pair"
    Pl = [[[float(P[o, s, j]) for s in range(k)] for j in range(da)] for o in range(nOrders)]  # [order][j][s] (:246-249)
    wl = list(map(float, w))

    A = [[[1.0 if t == 0 else 0.0] * k for _ in range(n)] for t in range(degree + 1)]
    dA = [[[0.0] * k for _ in range(n)] for _ in range(degree)]

    colNormSq = [0.0] * d
    if fitLinear:
        for j in range(d):
            acc = 0.0
            for _, v in cols[j]:
                acc += v * v
            r = math.sqrt(acc)
            colNormSq[j] = r * r

    yPred = [0.0] * n
    for j in range(d):
        for i, v in cols[j]:
            yPred[i] += v * wl[j]
    for i in range(n):
        yPred[i] += b

    def precompute_anova(Po, deg):  # :61-77: always the general recursion, product order (A * val) * P
        for t in range(1, deg + 1):
            for i in range(n):
                for s in range(k):
                    A[t][i][s] = 0.0
        for j in range(da):
            pj = Po[j]
            for t in range(deg):
                hi, lw = A[deg - t], A[deg - t - 1]
                for i, v in cols_aug[j]:
                    for s in range(k):
                        hi[i][s] += lw[i][s] * v * pj[s]

    for o in range(nOrders):
        precompute_anova(Pl[o], degree - o)
        top = A[degree - o]
        for i in range(n):
            for s in range(k):
                yPred[i] += top[i][s]

    def epoch(Po, deg, lossVal):
        res = 0.0
        R.compute_cache(Po)

        def phase_a(j):  # update (:112-152) up to the gradient step: nothing here reads the regulariser
            pj = Po[j]
            col = cols_aug[j]
            if deg > 2:
                for i, v in col:
                    for s in range(k):
                        dA[0][i][s] = v
                for g in range(1, deg):
                    for i, v in col:
                        for s in range(k):
                            dA[g][i][s] = v * (A[g][i][s] - pj[s] * dA[g - 1][i][s])
            else:
                for i, v in col:
                    for s in range(k):
                        dA[1][i][s] = v * (A[1][i][s] - v * pj[s])
            grad, invs = [0.0] * k, [0.0] * k
            top = dA[deg - 1]
            if pair and j >= d:
                dLs = [dl(y[i], yPred[i]) for i, _ in col]
                for s in range(k):
                    grad[s] = total([dL * top[i][s] for dL, (i, _) in zip(dLs, col)], sums)
                    invs[s] = total([top[i][s] * top[i][s] for i, _ in col], sums)
                col = []
            for i, v in col:
                dL = dl(y[i], yPred[i])
                for s in range(k):
                    grad[s] += dL * top[i][s]
                    invs[s] += top[i][s] * top[i][s]
            for s in range(k):
                grad[s] /= nf
            for s in range(k):
                grad[s] += beta * pj[s]
            acc = 0.0
            for s in range(k):
                acc += invs[s]
            inv = acc * mu / nf
            inv += beta
            inv = max(inv, 1e-12)
            old = list(pj)
            return old, [pj[s] - grad[s] / inv for s in range(k)], inv

        def phase_b(j, old, u, inv):  # the prox, the cache hook, delta = old - new (:154-157)
            pj = Po[j]
            for s in range(k):
                pj[s] = u[s]
            R.prox(pj, gamma / inv, j)
            R.update_cache(pj, j)
            return [-pj[s] + old[s] for s in range(k)]

        def phase_c(j, delta, lossVal):  # :184-206
            top = dA[deg - 1]
            for i, v in cols_aug[j]:
                lossVal -= lo(y[i], yPred[i])
                dot = 0.0
                for s in range(k):
                    dot += delta[s] * top[i][s]
                yPred[i] -= dot
                lossVal += lo(y[i], yPred[i])
            if deg == 2:
                for i, v in cols_aug[j]:
                    for s in range(k):
                        A[1][i][s] -= v * delta[s]
            else:
                for g in range(1, deg):  # A[deg] is left as it is
                    for i, v in cols_aug[j]:
                        for s in range(k):
                            A[g][i][s] -= dA[g - 1][i][s] * delta[s]
            return lossVal

        viols = [0.0] * da
        for group in groups:
            pre = [(j,) + phase_a(j) for j in group]
            steps = []
            for j, old, u, inv in pre:
                delta = phase_b(j, old, u, inv)
                viols[j] = norm1(delta)
                steps.append((j, delta))
            for j, delta in reversed(steps):
                lossVal = phase_c(j, delta, lossVal)
        for j in range(da):
            res += viols[j]
        return res, lossVal

    history = []
    converged = False
    for it in range(maxIter):
        viol = 0.0
        if fitIntercept:  # fitInterceptCD
            r = a0n * b
            if pair:
                r += total([dl(y[i], yPred[i]) for i in range(n)], sums)
            else:
                for i in range(n):
                    r += dl(y[i], yPred[i])
            r /= mu * nf + a0n
            b -= r
            for i in range(n):
                yPred[i] -= r
            viol += abs(r)
        if fitLinear:  # fitLinearCD
            res = 0.0
            viol_w = [0.0] * d
            for j in w_order:
                update = an * wl[j]
                for i, v in cols[j]:
                    update += dl(y[i], yPred[i]) * v
                inv = mu * colNormSq[j] + an
                if inv < 1e-12:
                    continue
                update /= inv
                viol_w[j] = abs(update)
                wl[j] -= update
                for i, v in cols[j]:
                    yPred[i] -= update * v
            for j in range(d):
                res += viol_w[j]
            viol += res
        lossVal = 0.0
        for i in range(n):
            lossVal += lo(y[i], yPred[i])
        if nOrders == 1:
            r, lossVal = epoch(Pl[0], degree, lossVal)
            viol += r
        else:
            for o in range(nOrders):
                precompute_anova(Pl[o], degree - o)
                r, lossVal = epoch(Pl[o], degree - o, lossVal)
                viol += r
        if pair:
            lossVal = total([lo(y[i], yPred[i]) for i in range(n)], sums)
        history.append((viol, lossVal / nf))
        Pout = np.array(Pl, dtype=np.float64).reshape(nOrders, da, k).transpose(0, 2, 1).copy()
        if callback is not None:
            callback(it, Pout, np.array(wl), b)
        if viol < tol:
            converged = True
            break
    last_resums = R.resums
    Pout = np.array(Pl, dtype=np.float64).reshape(nOrders, da, k).transpose(0, 2, 1).copy()
    return Pout, np.array(wl, dtype=np.float64), b, history, converged
