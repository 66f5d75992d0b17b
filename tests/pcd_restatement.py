"""Plain-Python restatement of the reference's proximal coordinate descent: optimizer/pcd.nim `fit` (:110-201) with
`epochDeg2` (:77-107) and `epoch` (:38-74), and the CD hooks of the four PCD regularisers: L1 (l1.nim:25-27,44,58-60),
SquaredL12 (squaredl12.nim:127-131,164-188; transpose=True is the default, one running cache per component, transpose=False
one cache per feature) and OmegaTI (omegati.nim:33-66).  Python floats are IEEE doubles and Python never fuses a
multiply-add, so every sum and product is rounded as in the reference's generated C.

order="reference" walks the features in ascending j.  order="level" walks the P sweep in CD's level schedule, reversed
inside each level (cd.hip): right for L1 and row-wise SquaredL12, wrong for the chained regularisers, whose prox reads a
running value over every earlier feature.  order="run" walks the run schedule of the library: runs
of consecutive features that share no sample; per run, every gradient from the state before the run, then the proximal
chain in ascending j, then the synchronisations (here in reverse).  The intercept, the w sweep and the dummy features keep
the reference's sums here; the device sums the intercept and the dummies with a fixed tree.  sums="pair" takes those sums and the loss's with np.sum, as
tests/cd_restatement.py does.
"""
import math

import numpy as np

from cd_restatement import _div, columns, levels, loss_fns, total  # noqa: F401


def softthreshold(x, a):
    """regularizer/utils.nim:4-5: float64(sgn(x)) * max(abs(x) - a, 0.0)"""
    x, a = float(x), float(a)
    sg = float((x > 0) - (x < 0))
    m = abs(x) - a
    return sg * (m if m > 0.0 else 0.0)


class Reg:
    """one regulariser's CD hooks and prox, state included (initCD, computeCacheCDAll, computeCacheCD, prox, updateCacheCD)"""

    def __init__(self, name, transpose=True, degree=2, nFeatures=0):
        self.name, self.transpose = name, bool(transpose)
        if name == "squaredl12" and degree != 2:  # initCD, squaredl12.nim:90-93
            raise ValueError("SquaredL12 supports only degree=2.")
        self.absp = [0.0] * nFeatures
        if name == "squaredl12":
            self.cache = [0.0] * (1 if self.transpose else nFeatures)
        elif name == "omegati":
            self.cache = [0.0] * (degree + 1)
            self.dcache = [0.0] * (degree + 1)

    @property
    def chained(self):
        return self.name == "omegati" or (self.name == "squaredl12" and self.transpose)

    def cache_all(self, Po):  # computeCacheCDAll, Po [k][d + nAug]
        if self.name == "squaredl12" and not self.transpose:
            for j in range(len(self.cache)):
                self.cache[j] = 0.0
            for s in range(len(Po)):
                for j in range(len(self.cache)):
                    self.cache[j] += abs(Po[s][j])

    def cache_comp(self, Ps, degree):  # computeCacheCD
        if self.name == "l1":
            return
        for j in range(len(Ps)):
            self.absp[j] = abs(Ps[j])
        if self.name == "squaredl12":
            if self.transpose:
                acc = 0.0
                for v in self.absp:
                    acc += v
                self.cache[0] = acc
            return
        for t in range(1, len(self.cache)):
            self.cache[t] = 0.0
        self.cache[0] = 1.0
        for t in range(len(self.dcache)):
            self.dcache[t] = 0.0
        self.dcache[1] = 1.0
        for j in range(len(Ps)):
            for deg in range(degree):
                self.cache[degree - deg] += self.cache[degree - deg - 1] * abs(Ps[j])

    def prox(self, psj, update, lam, degree, j):
        if self.name == "l1":
            return softthreshold(psj - update, lam)
        if self.name == "squaredl12":
            i = 0 if self.transpose else j
            dcache = self.cache[i] - self.absp[j]
            return softthreshold((psj - update) / (1 + 2 * lam), 2 * lam * dcache / (1 + 2 * lam))
        for deg in range(2, degree + 1):  # omegati.nim:58-66
            self.dcache[deg] = self.cache[deg - 1] - self.dcache[deg - 1] * self.absp[j]
            if self.dcache[deg] < 0:
                self.dcache[deg] = 0.0
        return softthreshold(psj - update, lam * self.dcache[degree])

    def update_cache(self, pnew, degree, j):  # updateCacheCD
        if self.name == "squaredl12":
            i = 0 if self.transpose else j
            self.cache[i] -= self.absp[j]
            self.cache[i] += abs(pnew)
        elif self.name == "omegati":
            for deg in range(1, degree):
                self.cache[deg] = self.dcache[deg + 1] + self.dcache[deg] * abs(pnew)


def runs(cols):
    """the run schedule: walk j ascending, cut a new run when column j shares a sample with a column of the current run"""
    out, cur, seen = [], [], set()
    for j, col in enumerate(cols):
        rows = {i for i, _ in col}
        if rows & seen:
            out.append(cur)
            cur, seen = [], set()
        cur.append(j)
        seen |= rows
    if cur:
        out.append(cur)
    return out


def schedule(indptr, indices, n, d, chained):
    """(number of runs or levels, the widest) of the real features, as nfm_cd_schedule reports them without augments"""
    cols = columns(indptr, indices, np.ones(len(indices)), n, d)
    if chained:
        rs = runs(cols)
        return len(rs), max((len(r) for r in rs), default=0)
    counts = {}
    for v in levels(cols, n):
        counts[v] = counts.get(v, 0) + 1
    return len(counts), max(counts.values()) if counts else 0


def fit(indptr, indices, data, y, P, w, intercept, degree, nAugments, fitLinear, fitIntercept, maxIter=100, alpha0=1e-6,
        alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", lossParam=1.0, tol=1e-3, task="regression", reg="squaredl12",
        transpose=True, order="reference", callback=None, sums="seq"):
    """-> (P, w, intercept, history, converged); P [nOrders][k][d + nAugments] (copied), history [(viol, mean loss)]"""
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
    a0n, an, bn, gn = alpha0 * float(n), alpha * float(n), beta * float(n), gamma * float(n)
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
    Pl = [[list(map(float, P[o, s])) for s in range(k)] for o in range(nOrders)]
    wl = list(map(float, w))

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

    def anova(Ps, deg):
        A = [[1.0] + [0.0] * deg for _ in range(n)]
        if deg != 2:
            for j in range(da):
                for i, v in cols_aug[j]:
                    Ai = A[i]
                    for t in range(deg):
                        Ai[deg - t] += Ai[deg - t - 1] * Ps[j] * v
        else:
            for j in range(da):
                for i, v in cols_aug[j]:
                    A[i][1] += Ps[j] * v
                    t = Ps[j] * v
                    A[i][2] += t * t
            for i in range(n):
                A[i][2] = (A[i][1] * A[i][1] - A[i][2]) / 2.0
        return A

    for o in range(nOrders):
        for s in range(k):
            A = anova(Pl[o][s], degree - o)
            for i in range(n):
                yPred[i] += A[i][degree - o]

    history = []
    converged = False
    pair = sums == "pair"
    for it in range(maxIter):
        viol = 0.0
        if fitIntercept:
            r = a0n * b
            if pair:
                r += total([dl(y[i], yPred[i]) for i in range(n)], sums)
            else:
                for i in range(n):
                    r += dl(y[i], yPred[i])
            r /= mu * float(n) + a0n
            b -= r
            for i in range(n):
                yPred[i] -= r
            viol += abs(r)
        if fitLinear:
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
        for o in range(nOrders):
            deg = degree - o
            res = 0.0
            vs = [[0.0] * da for _ in range(k)]
            R.cache_all(Pl[o])
            for s in range(k):
                Ps = Pl[o][s]
                if deg == 2:
                    cache = [0.0] * n
                    for j in range(da):
                        for i, v in cols_aug[j]:
                            cache[i] += v * Ps[j]
                else:
                    A = anova(Ps, deg)
                R.cache_comp(Ps, deg)

                def grad(j):
                    psj = Ps[j]
                    update, inv = bn * psj, 0.0
                    t1, t2 = [], []
                    for i, v in cols_aug[j]:
                        if deg == 2:
                            top = (cache[i] - psj * v) * v
                        else:
                            Ai = A[i]
                            dA = [v] + [0.0] * (deg - 1)
                            for g in range(1, deg):
                                dA[g] = v * (Ai[g] - psj * dA[g - 1])
                            top = dA[deg - 1]
                        if pair and j >= d:
                            t1.append(dl(y[i], yPred[i]) * top)
                            t2.append(top * top)
                            continue
                        update += dl(y[i], yPred[i]) * top
                        inv += top * top
                    if pair and j >= d:
                        update += total(t1, sums)
                        inv = total(t2, sums)
                    if deg == 2:
                        inv = inv * mu + bn
                    else:
                        inv *= mu
                        inv += bn
                    return psj, update, inv

                def sync(j, psj, update):
                    for i, v in cols_aug[j]:
                        if deg == 2:
                            yPred[i] -= update * (cache[i] - psj * v) * v
                            cache[i] -= update * v
                        else:
                            Ai = A[i]
                            dA = [v] + [0.0] * (deg - 1)
                            for g in range(1, deg):
                                dA[g] = v * (Ai[g] - psj * dA[g - 1])
                                Ai[g] -= update * dA[g - 1]
                            Ai[deg] -= update * dA[deg - 1]
                            yPred[i] -= update * dA[deg - 1]

                for group in groups:
                    grads = [(j,) + grad(j) for j in group]  # every gradient of the group before any step
                    steps = []
                    for j, psj, update, inv in grads:
                        if inv < 1e-12:  # pcd.nim:57,100: neither prox nor updateCacheCD
                            continue
                        update /= inv
                        Ps[j] = R.prox(psj, update, gn / inv, deg, j)
                        update = psj - Ps[j]
                        vs[s][j] = abs(update)
                        R.update_cache(Ps[j], deg, j)
                        steps.append((j, psj, update))
                    for j, psj, update in reversed(steps):
                        sync(j, psj, update)
            for s in range(k):
                for j in range(da):
                    res += vs[s][j]
            viol += res
        lossVal = total([lo(y[i], yPred[i]) for i in range(n)], sums)
        history.append((viol, lossVal / float(n)))
        if callback is not None:
            callback(it, np.array(Pl), np.array(wl), b)
        if viol < tol:
            converged = True
            break
    return np.array(Pl, dtype=np.float64).reshape(nOrders, k, da), np.array(wl, dtype=np.float64), b, history, converged
