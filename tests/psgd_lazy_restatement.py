"""A plain-Python restatement of the reference's PSGD with its lazily updated regularisers, line by line and independent of
oracle/: optimizer/psgd.nim:58-215 (finalize and fit), the SGD hooks of regularizer/l1.nim:47-52,80-136 and
regularizer/l21.nim:38-43,64-113, predictWithGrad (optimizer/sgd.nim:146-202), getEta (sgd.nim:60-69), fitLinearSGD
(fit_linear.nim:41-47), the losses (loss.nim) and softthreshold (regularizer/utils.nim:4-5); and the dense solver the
reference tests it against, PSGDSlow (tests/optimizer/psgd_slow.nim:43-99 with tests/model/fm_slow.nim:42-60,111-134).

Element-wise work on a feature's factors is done with numpy (every element rounds as the scalar loop's does); every SUM
whose order matters -- over the row's entries, over the factors -- is a Python loop in the reference's order.

Two switches the reference does not have:
  l1_reset = "reference": L1's resetCacheSGD as written (l1.nim:113-126); "consistent": lazyUpdateFinal's formula on every
             row, then the cache reset -- what finalize does and what L21's own reset does (the device does this).
  resets = False: no cache reset and no reset of w at all.

A Record collects, for every soft threshold and every group threshold taken, the relative distance between the thresholded
magnitude and the threshold (the smallest one bounds how far a rounding difference may be from flipping a zero), and how
many cache resets and w resets ran."""
import itertools
import math

import numpy as np


# ---- model/factorization_machine.nim:81-97 ----
def n_augments(degree, fit_lower, fit_linear):
    if fit_lower in ("explicit", "none"):
        return 0
    return degree - 2 if fit_linear else degree - 1


def n_orders(degree, fit_lower):
    if degree == 1:
        return 0
    return degree - 1 if fit_lower == "explicit" else 1


class Record:
    def __init__(self):
        self.min_margin = float("inf")
        self.cache_resets = 0
        self.w_resets = 0
        self.thresholds_taken = 0

    def see(self, magnitude, threshold):
        """magnitude: array (soft threshold) or scalar (a row's norm)"""
        mag = np.abs(np.atleast_1d(np.asarray(magnitude, dtype=np.float64)))
        thr = abs(float(threshold))
        scale = np.maximum(mag, thr)
        live = scale > 0.0  # 0 against 0 is 0 however it is rounded
        if live.any():
            self.min_margin = min(self.min_margin, float((np.abs(mag[live] - thr) / scale[live]).min()))
        self.thresholds_taken += int(mag.size)


def softthreshold(x, alpha, rec=None):
    """regularizer/utils.nim:4-5: float64(sgn(x)) * max(abs(x) - alpha, 0.0), element-wise"""
    if rec is not None:
        rec.see(x, alpha)
    return np.sign(x) * np.maximum(np.abs(x) - alpha, 0.0)


def norm2(v):
    """tensor.nim:608-616 norm(v, 2): the in-order sum of |x|^2; the root is taken with sqrt (correctly rounded)"""
    acc = 0.0
    for x in v:
        acc += abs(float(x)) * abs(float(x))
    return math.sqrt(acc)


# ---- loss.nim ----
def loss_value(name, param, y, p):
    if name == "squared":  # :18
        return 0.5 * ((y - p) * (y - p))
    if name == "squared_hinge":  # :33
        m = max(1 - p * y, 0.0)
        return m * m
    if name == "logistic":  # :54-59
        z = p * y
        if z > 0:
            return math.log(1 + math.exp(-z))
        return math.log(math.exp(z) + 1) - z
    z = abs(y - p)  # Huber :84-87
    if z < param:
        return 0.5 * (z * z)
    return param * (z - 0.5 * param)


def loss_grad(name, param, y, p):
    if name == "squared":  # :21
        return p - y
    if name == "squared_hinge":  # :36-39
        z = 1 - p * y
        return -2 * y * z if z > 0 else 0.0
    if name == "logistic":  # :62-67
        z = p * y
        if z > 0:
            return -y * math.exp(-z) / (1 + math.exp(-z))
        return -y / (math.exp(z) + 1)
    z = abs(y - p)  # Huber :90-93, its sign as written
    return y - p if z < param else param


def get_eta(cfg, reg, it):
    """sgd.nim:60-69"""
    s, eta0, power = cfg["scheduling"], cfg["eta0"], cfg["power"]
    if s == "constant":
        return eta0
    if s == "optimal":
        return eta0 / math.pow(1.0 + eta0 * reg * float(it), power)
    if s == "invscaling":
        return eta0 / math.pow(float(it), power)
    return 1.0 / (reg * float(it))  # pegasos


def check_target(y, task):
    """fm_base.nim:29-36"""
    y = np.asarray(y, dtype=np.float64)
    return np.sign(y) if task == "classification" else y.copy()


# ---- regularizer/l1.nim ----
class L1:
    name = "l1"

    def __init__(self, rec, l1_reset="consistent", resets=True):
        assert l1_reset in ("reference", "consistent")
        self.rec, self.l1_reset, self.resets = rec, l1_reset, resets

    def initSGD(self, nFeatures):  # :47-52
        self.scalings = np.ones(nFeatures)
        self.scaling = 1.0
        self.thresholds = np.zeros(nFeatures)
        self.threshold = 0.0

    def lazyUpdate(self, P, beta, gamma, row):  # :80-86, P: [nFeatures][nComponents]
        for j in row:
            P[j] *= self.scaling / self.scalings[j]
            P[j] = softthreshold(P[j], gamma * self.scaling * (self.threshold - self.thresholds[j]), self.rec)

    def lazyUpdateFinal(self, P, beta, gamma):  # :89-100, P: [nOrders][nFeatures][nComponents]
        for order in range(P.shape[0]):
            for j in range(P.shape[1]):
                P[order, j] *= self.scaling / self.scalings[j]
                P[order, j] = softthreshold(P[order, j], gamma * self.scaling * (self.threshold - self.thresholds[j]), self.rec)
        self.scalings[:] = 1.0
        self.scaling = 1.0
        self.thresholds[:] = 0.0
        self.threshold = 0.0

    def updateCacheSGD(self, eta, beta, gamma, row):  # :103-110
        eta_P_scaled = eta / (1 + eta * beta)
        self.threshold += eta_P_scaled / self.scaling
        self.scaling *= (1 - eta_P_scaled * beta)
        for j in row:
            self.scalings[j] = self.scaling
            self.thresholds[j] = self.threshold

    def resetCacheSGD(self, P, gamma):  # :113-126
        if not self.resets or not self.scaling < 1e-8:
            return
        self.rec.cache_resets += 1
        if self.l1_reset == "consistent":
            self.lazyUpdateFinal(P, 0.0, gamma)
            return
        for order in range(P.shape[0]):
            for j in range(P.shape[1]):
                P[order, j] /= self.scalings[j]
                P[order, j] = softthreshold(P[order, j], gamma * self.threshold - self.thresholds[j])
                P[order, j] *= self.threshold
        self.threshold = 0.0
        self.scaling = 1.0
        self.thresholds[:] = 0.0
        self.scalings[:] = 1.0

    def step(self, P, dA, dL, beta, gamma, eta_P_scaled, row):  # :129-136
        for j in row:
            update = eta_P_scaled * (dL * dA[j] + beta * P[j])
            P[j] = softthreshold(P[j] - update, gamma * eta_P_scaled, self.rec)

    def prox_dense(self, Pt, lam):  # :38-41, Pt: [nComponents][nFeatures] of the dense solver
        Pt[:] = softthreshold(Pt, lam)

    def eval(self, P):  # :18
        return float(np.abs(P).sum())


# ---- regularizer/l21.nim ----
class L21:
    name = "l21"

    def __init__(self, rec, l1_reset="consistent", resets=True):
        self.rec, self.resets = rec, resets

    def prox(self, pj, lam, record=True):  # :25-29
        norm = norm2(pj)
        if record:
            self.rec.see(norm, lam)
        if norm > lam:
            pj *= (1.0 - lam / norm)
        else:
            pj[:] = 0.0

    def initSGD(self, nFeatures):  # :38-43
        self.scalings = np.ones(nFeatures)
        self.thresholds = np.zeros(nFeatures)
        self.scaling = 1.0
        self.threshold = 0.0

    def lazyUpdate(self, P, beta, gamma, row):  # :64-69
        for j in row:
            threshold = (self.threshold - self.thresholds[j]) / self.scalings[j]
            self.prox(P[j], threshold * gamma)
            P[j] *= self.scaling / self.scalings[j]

    def lazyUpdateFinal(self, P, beta, gamma):  # :72-78 (the caches stay as they are: finalize is followed by initSGD or by more steps)
        for order in range(P.shape[0]):
            for j in range(P.shape[1]):
                threshold = (self.threshold - self.thresholds[j]) / self.scalings[j]
                self.prox(P[order, j], threshold * gamma)
                P[order, j] *= self.scaling / self.scalings[j]

    def updateCacheSGD(self, eta, beta, gamma, row):  # :81-87
        self.threshold += eta * self.scaling
        self.scaling /= (1 + eta * beta)
        for j in row:
            self.scalings[j] = self.scaling
            self.thresholds[j] = self.threshold

    def resetCacheSGD(self, P, gamma):  # :90-101
        if not self.resets or not self.scaling < 1e-8:
            return
        self.rec.cache_resets += 1
        self.lazyUpdateFinal(P, 0.0, gamma)
        self.threshold = 0.0
        self.scaling = 1.0
        self.thresholds[:] = 0.0
        self.scalings[:] = 1.0

    def step(self, P, dA, dL, beta, gamma, eta_P_scaled, row):  # :105-113
        for j in row:
            update = eta_P_scaled * (dL * dA[j] + beta * P[j])
            P[j] -= update
            self.prox(P[j], eta_P_scaled * gamma)

    def prox_dense(self, Pt, lam):  # :33-35 on the dense solver's [nComponents][nFeatures]
        for j in range(Pt.shape[1]):
            col = Pt[:, j].copy()
            self.prox(col, lam, record=False)
            Pt[:, j] = col

    def eval(self, P):  # :17-18
        return float(sum(norm2(P[j]) for j in range(P.shape[0])))


REGS = {"l1": L1, "l21": L21}


# ---- optimizer/sgd.nim:146-202 ----
def compute_anova(P, idx, val, degree, A):
    """:146-173, P: [nFeatures][nComponents], A: [nComponents][degree + 1]; -> sum over s ascending of A[s, degree]"""
    k = P.shape[1]
    if degree != 2:
        A[:, 0] = 1.0
        A[:, 1:degree + 1] = 0.0
        for j, v in zip(idx, val):
            for t in range(degree):
                A[:, degree - t] += A[:, degree - t - 1] * P[j] * v
    else:
        A[:, 0] = 1.0
        A[:, 1] = 0.0
        A[:, 2] = 0.0
        for j, v in zip(idx, val):
            A[:, 1] += v * P[j]
            A[:, 2] += (v * P[j]) * (v * P[j])
        A[:, 2] = (A[:, 1] * A[:, 1] - A[:, 2]) / 2
    result = 0.0
    for s in range(k):
        result += float(A[s, degree])
    return result


def compute_anova_derivative(P, idx, val, degree, A, dA):
    """:176-188"""
    if degree != 2:
        for j, v in zip(idx, val):
            dA[j] = v
            for t in range(1, degree):
                dA[j] = v * (A[:, t] - P[j] * dA[j])
    else:
        for j, v in zip(idx, val):
            dA[j] = v * (A[:, 1] - P[j] * v)


def predict_with_grad(idx, val, d, P, w, intercept, A, dA, degree, nAugments):
    """:191-202; idx, val: the row's entries in storage order"""
    result = intercept
    for j, v in zip(idx, val):
        result += float(w[j]) * float(v)
    idx_a = list(idx) + [d + t for t in range(nAugments)]  # addDummyFeature(1.0, nAugments), dataset.nim:182-189
    val_a = list(val) + [1.0] * nAugments
    for order in range(P.shape[0]):
        result += compute_anova(P[order], idx_a, val_a, degree - order, A)
        compute_anova_derivative(P[order], idx_a, val_a, degree - order, A, dA[order])
    return result


class Result:
    pass


def psgd_fit(indptr, indices, data, n, d, y, P0, w0, b0, *, task="regression", degree=2, fit_lower="explicit", fit_linear=True,
             fit_intercept=True, reg="l1", maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared",
             loss_param=1.0, scheduling="optimal", power=1.0, tol=1e-3, perms=None, nCalls=-1, callback=None, it=1,
             l1_reset="consistent", resets=True, finalize_at_end=True):
    """psgd.nim:76-215.  P0: fm.P [nOrders][nComponents][nFeatures + nAugments].  perms: [maxIter][n] or None (the dataset's order:
    shuffle = false).  callback(it, P, w, b) gets the finalized model.  -> Result: P, w, intercept (fm's layouts), it, losses (the
    per-epoch running loss SUMS), record, caches (scalings, thresholds, scalings_w, scaling, threshold, scaling_w)"""
    cfg = dict(eta0=eta0, scheduling=scheduling, power=power)
    rec = Record()
    r = REGS[reg](rec, l1_reset, resets)
    y = check_target(y, task)
    nAugments = n_augments(degree, fit_lower, fit_linear)
    fmP = np.array(P0, dtype=np.float64)
    nOrders, nComponents = fmP.shape[0], fmP.shape[1]
    w = np.array(w0, dtype=np.float64)
    b = float(b0)
    scaling_w = 1.0  # :97-98
    scalings_w = np.ones(d)
    A = np.zeros((nComponents, degree + 1))
    P = np.ascontiguousarray(fmP.transpose(0, 2, 1))  # :109-110: [nOrders][nFeatures + nAugments][nComponents]
    dA = np.zeros(P.shape)
    r.initSGD(d + nAugments)  # :112
    res = Result()

    def finalize():  # :58-73
        nonlocal w
        if fit_linear:
            w *= scaling_w
            w /= scalings_w
            scalings_w[:] = scaling_w
        r.lazyUpdateFinal(P, beta, gamma)
        fmP[:] = P.transpose(0, 2, 1)

    losses = []
    runningLossOld = 0.0
    res.converged_at = None
    for epoch in range(maxIter):
        runningLoss = 0.0
        order_ = perms[epoch] if perms is not None else range(n)
        for i in order_:
            i = int(i)
            idx = [int(j) for j in indices[indptr[i]:indptr[i + 1]]]
            val = [float(v) for v in data[indptr[i]:indptr[i + 1]]]
            idx_a = idx + [d + t for t in range(nAugments)]
            for j in idx:  # :124-125
                w[j] *= scaling_w / scalings_w[j]
            for order in range(nOrders):  # :126-129
                r.lazyUpdate(P[order], beta, gamma, idx_a)
            yPred = predict_with_grad(idx, val, d, P, w, b, A, dA, degree, nAugments)
            runningLoss += loss_value(loss, loss_param, float(y[i]), yPred)  # :132
            eta_w = get_eta(cfg, alpha, it)  # :135-138
            eta_P = get_eta(cfg, beta, it)
            eta_P_scaled = eta_P / (1.0 + eta_P * beta)
            dL = loss_grad(loss, loss_param, float(y[i]), yPred)
            for order in range(nOrders):  # :141-145
                r.step(P[order], dA[order], dL, beta, gamma, eta_P_scaled, idx_a)
            r.updateCacheSGD(eta_P, beta, gamma, idx_a)  # :146
            if fit_intercept:  # :150-152
                update = get_eta(cfg, alpha0, it) * (dL + alpha0 * b)
                b -= update / (1.0 + get_eta(cfg, alpha0, it) * alpha0)
            if fit_linear:  # :153-154, fit_linear.nim:41-47
                eta = eta_w / (1.0 + eta_w * alpha)
                for j, v in zip(idx, val):
                    update = eta * (dL * v + alpha * w[j])
                    w[j] -= update
            scaling_w /= (1.0 + eta_w * alpha)  # :157-159
            for j in idx:
                scalings_w[j] = scaling_w
            if resets and fit_linear and scaling_w < 1e-9:  # :162-166
                rec.w_resets += 1
                w *= scaling_w
                w /= scalings_w
                scalings_w[:] = 1.0
                scaling_w = 1.0
            r.resetCacheSGD(P, gamma)  # :167
            for order in range(nOrders):  # :170-176
                for j in idx_a:
                    dA[order, j] = 0.0
            if nCalls > 0 and it % nCalls == 0 and callback is not None:  # :179-182
                finalize()
                callback(it, fmP.copy(), w.copy(), b)
            it += 1  # :184
        losses.append(runningLoss)
        runningLoss /= float(n)  # :186
        if callback is not None and nCalls <= 0:  # :190-192
            finalize()
            callback(it, fmP.copy(), w.copy(), b)
        if math.isnan(runningLoss):  # :194-196
            break
        if abs(runningLoss - runningLossOld) < tol:  # :198-201
            res.converged_at = epoch
            break
        runningLossOld = runningLoss
    res.caches = dict(scalings=r.scalings.copy(), thresholds=r.thresholds.copy(), scalings_w=scalings_w.copy(), scaling=r.scaling,
                      threshold=r.threshold, scaling_w=scaling_w)
    if finalize_at_end:
        finalize()  # :215
    else:
        fmP[:] = P.transpose(0, 2, 1)
    res.P, res.w, res.intercept, res.it, res.losses, res.record = fmP, w, b, it, losses, rec
    return res


# ---- tests/optimizer/psgd_slow.nim:43-99 with tests/model/fm_slow.nim ----
def _combos(D, degree):
    return np.array(list(itertools.combinations(range(D), degree)), dtype=np.int64).reshape(-1, degree)


def psgd_slow_fit(Xd, y, P0, w0, b0, *, task="regression", degree=2, fit_lower="explicit", fit_linear=True, fit_intercept=True,
                  reg="l1", maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", loss_param=1.0,
                  scheduling="optimal", power=1.0, perms=None, it=1):
    """The dense solver: every parameter steps at every sample and the regulariser's prox follows (no laziness).  The sums over
    index combinations (fm_slow.nim:53-60,123-129) are taken with numpy: the comparison it serves is at 1e-6."""
    cfg = dict(eta0=eta0, scheduling=scheduling, power=power)
    r = REGS[reg](Record())
    Xd = np.asarray(Xd, dtype=np.float64)
    n, d = Xd.shape
    y = check_target(y, task)
    nAugments = n_augments(degree, fit_lower, fit_linear)
    P = np.array(P0, dtype=np.float64)  # [nOrders][nComponents][d + nAugments]
    nOrders, k, D = P.shape
    w = np.array(w0, dtype=np.float64)
    b = float(b0)
    combos = {}
    for order in range(nOrders):
        deg = degree - order
        combos[order] = (_combos(D, deg), [np.array([c for c in itertools.combinations([t for t in range(D) if t != j], deg - 1)],
                                                    dtype=np.int64).reshape(-1, deg - 1) for j in range(D)])
    for epoch in range(maxIter):
        order_ = perms[epoch] if perms is not None else range(n)
        for i in order_:
            i = int(i)
            xa = np.concatenate([Xd[i], np.ones(nAugments)])
            yPred = b + float(np.dot(w, Xd[i]))  # fm_slow.nim:47-60
            Z = P * xa  # [nOrders][k][D]
            for order in range(nOrders):
                yPred += float(np.prod(Z[order][:, combos[order][0]], axis=2).sum())
            dL = loss_grad(loss, loss_param, float(y[i]), yPred)
            grad = np.zeros(P.shape)  # fm_slow.nim:111-134
            for order in range(nOrders):
                for j in range(D):
                    c = combos[order][1][j]
                    tmp = np.prod(Z[order][:, c], axis=2).sum(axis=1) if c.shape[1] > 0 else np.ones(k)
                    grad[order, :, j] = dL * (tmp * xa[j])
            eta_w = get_eta(cfg, alpha, it)  # psgd_slow.nim:81-98
            eta_P = get_eta(cfg, beta, it)
            eta_P_scaled = eta_P / (1.0 + eta_P * beta)
            if fit_intercept:
                update = get_eta(cfg, alpha0, it) * (dL + alpha0 * b)
                b -= update / (1.0 + get_eta(cfg, alpha0, it) * alpha0)
            if fit_linear:
                update = eta_w * (dL * Xd[i] + alpha * w)
                w -= update / (1.0 + eta_w * alpha)
            for order in range(nOrders):
                P[order] -= eta_P_scaled * (grad[order] + beta * P[order])
                r.prox_dense(P[order], gamma * eta_P_scaled)
            it += 1
    res = Result()
    res.P, res.w, res.intercept, res.it = P, w, b, it
    return res
