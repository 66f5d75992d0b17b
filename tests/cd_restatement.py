"""Plain-Python restatement of the reference's coordinate descent: optimizer/cd.nim `fit` (:128-183) with `epochDeg2`
(:77-107) and `epoch` (:50-74), fitLinearCD / fitInterceptCD (optimizer/fit_linear.nim:5-37), anova and linear over a
ColDataset (kernels.nim:4-43).  Python floats are IEEE doubles and Python never fuses a multiply-add, so every sum and
product is rounded as in the reference's generated C.

level_order=True walks the features of the w and P sweeps in the level schedule of the library (cd.hip) instead of
ascending j, with the features of each level in REVERSE: the claim the device kernels rest on is that this changes nothing.
The intercept and the dummy features (fitLower = augment) keep the reference's sums here; the device sums them with a
fixed tree.

sums="pair" takes exactly those sums -- the intercept's, the dummy features' and the loss's, each over every sample -- with
np.sum (pairwise) instead of one term after the other: the distance between the two is the spread a fixed tree on the
device may show (tests/test_cd_schedule_cases.py measures it).  Every other sum keeps the reference's order.
"""
import math

import numpy as np


def loss_fns(loss, threshold=1.0):
    """loss.nim: (loss, dloss, mu)"""
    if loss == "squared":
        return (lambda y, p: 0.5 * ((y - p) * (y - p))), (lambda y, p: p - y), 1.0
    if loss == "squared_hinge":
        def lo(y, p):
            m = max(1 - p * y, 0)
            return m * m

        def dl(y, p):
            z = 1 - p * y
            return -2 * y * z if z > 0 else 0.0
        return lo, dl, 2.0
    if loss == "logistic":
        def lo(y, p):
            z = p * y
            return math.log(1 + math.exp(-z)) if z > 0 else math.log(math.exp(z) + 1) - z

        def dl(y, p):
            z = p * y
            return -y * math.exp(-z) / (1 + math.exp(-z)) if z > 0 else -y / (math.exp(z) + 1)
        return lo, dl, 0.25
    if loss == "huber":
        def lo(y, p):
            z = abs(y - p)
            return 0.5 * (z * z) if z < threshold else threshold * (z - 0.5 * threshold)

        def dl(y, p):
            z = abs(y - p)
            return y - p if z < threshold else threshold
        return lo, dl, 1.0
    raise ValueError(loss)


def _div(a, b):
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def columns(indptr, indices, data, n, d):
    """the column twin: per feature, (sample, value) in ascending sample order"""
    cols = [[] for _ in range(d)]
    for i in range(n):
        for q in range(int(indptr[i]), int(indptr[i + 1])):
            cols[int(indices[q])].append((i, float(data[q])))
    return cols


def levels(cols, n):
    """level(j) = 1 + max(last[i] for i in col j) (0 for an empty column), then last[i] = level(j)"""
    last = [0] * n
    lv = []
    for col in cols:
        if not col:
            lv.append(0)
            continue
        m = max(last[i] for i, _ in col) + 1
        for i, _ in col:
            last[i] = m
        lv.append(m)
    return lv


def schedule_depth(indptr, indices, n, d):
    """(number of non-empty levels, widest level) of the real features"""
    cols = columns(indptr, indices, np.ones(len(indices)), n, d)
    lv = levels(cols, n)
    counts = {}
    for v in lv:
        counts[v] = counts.get(v, 0) + 1
    return len(counts), max(counts.values()) if counts else 0


def total(terms, sums):
    """the sum of a list of floats: one after the other from 0.0 ("seq"), or np.sum's pairwise tree ("pair")"""
    if sums == "pair":
        return float(np.sum(np.array(terms, dtype=np.float64)))
    acc = 0.0
    for t in terms:
        acc += t
    return acc


def _order(cols, n, level_order):
    d = len(cols)
    if not level_order:
        return list(range(d))
    lv = levels(cols, n)
    return sorted(range(d), key=lambda j: (lv[j], -j))


def fit(indptr, indices, data, y, P, w, intercept, degree, nAugments, fitLinear, fitIntercept, maxIter=100, alpha0=1e-6,
        alpha=1e-3, beta=1e-3, loss="squared", lossParam=1.0, tol=1e-3, task="regression", level_order=False, callback=None, sums="seq"):
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
    a0n, an, bn = alpha0 * float(n), alpha * float(n), beta * float(n)
    order = _order(cols, n, level_order)
    order_aug = order + list(range(d, d + nAugments))  # the dummy features: one level each, after all real features
    Pl = [[list(map(float, P[o, s])) for s in range(k)] for o in range(nOrders)]
    wl = list(map(float, w))

    colNormSq = [0.0] * d
    if fitLinear:
        for j in range(d):
            acc = 0.0
            for _, v in cols[j]:
                acc += v * v
            r = math.sqrt(acc)  # pow(acc, 1 / 2) (extmath.nim:163)
            colNormSq[j] = r * r

    # linear (kernels.nim:4-11) + intercept + anova per order and component (cd.nim:143-151)
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
                    A[i][2] += t * t  # (P[s, j] * val)^2: Nim's ^ multiplies
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
        if fitIntercept:  # fitInterceptCD
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
        if fitLinear:  # fitLinearCD
            res = 0.0
            viol_w = [0.0] * d
            for j in order:
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
            for j in range(d):  # the reference's order of the sum
                res += viol_w[j]
            viol += res
        for o in range(nOrders):
            deg = degree - o
            res = 0.0
            vs = [[0.0] * da for _ in range(k)]
            for s in range(k):
                Ps = Pl[o][s]
                if deg == 2:  # epochDeg2
                    cache = [0.0] * n
                    for j in range(da):
                        for i, v in cols_aug[j]:
                            cache[i] += v * Ps[j]
                    for j in order_aug:
                        psj = Ps[j]
                        update = bn * psj
                        inv = 0.0
                        if pair and j >= d:
                            dAs = [(cache[i] - psj * v) * v for i, v in cols_aug[j]]
                            update += total([dl(y[i], yPred[i]) * t for (i, _), t in zip(cols_aug[j], dAs)], sums)
                            inv = total([t * t for t in dAs], sums)
                        else:
                            for i, v in cols_aug[j]:
                                dA = (cache[i] - psj * v) * v
                                update += dl(y[i], yPred[i]) * dA
                                inv += dA * dA
                        inv = inv * mu + bn
                        if inv < 1e-12:
                            continue
                        update /= inv
                        vs[s][j] = abs(update)
                        for i, v in cols_aug[j]:
                            yPred[i] -= update * (cache[i] - psj * v) * v
                            cache[i] -= update * v
                        Ps[j] -= update
                else:  # epoch
                    A = anova(Ps, deg)
                    for j in order_aug:
                        psj = Ps[j]
                        update, inv = bn * psj, 0.0
                        t1, t2 = [], []
                        for i, v in cols_aug[j]:
                            Ai = A[i]
                            dA = [v] + [0.0] * (deg - 1)
                            for g in range(1, deg):
                                dA[g] = v * (Ai[g] - psj * dA[g - 1])
                            if pair and j >= d:
                                t1.append(dl(y[i], yPred[i]) * dA[deg - 1])
                                t2.append(dA[deg - 1] * dA[deg - 1])
                                continue
                            update += dl(y[i], yPred[i]) * dA[deg - 1]
                            inv += dA[deg - 1] * dA[deg - 1]
                        if pair and j >= d:
                            update += total(t1, sums)
                            inv = total(t2, sums)
                        inv *= mu
                        inv += bn
                        update = _div(update, inv)  # no guard here (cd.nim:59-61): IEEE division, as in the reference
                        Ps[j] -= update
                        vs[s][j] = abs(update)
                        for i, v in cols_aug[j]:
                            Ai = A[i]
                            dA = [v] + [0.0] * (deg - 1)
                            for g in range(1, deg):
                                dA[g] = v * (Ai[g] - psj * dA[g - 1])
                                Ai[g] -= update * dA[g - 1]
                            Ai[deg] -= update * dA[deg - 1]
                            yPred[i] -= update * dA[deg - 1]
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
