"""Hazan's algorithm for the convex factorization machine, restated from the reference in its own loop order:
optimizer/hazan.nim:59-225, tensor/tensor.nim:912-934 (powerMethod) and :970-1009 (cg), kernels.nim:22-43 (anova) and
:67-79 (poly), extmath.nim:93-123 (mvmul / vmmul of a column dataset).  No GPU, no library: numpy only.

Sums along a row or a column are taken entry after entry in storage order, as the reference's loops (and the device's row
and column passes) take them.  The vector reductions -- the dot products and norms over nSamples or nFeatures -- are
switchable: summation="order" adds in index order as the reference does, summation="tree" follows the device's fixed trees
(per workgroup a halving tree over 32 rows / columns or 256 elements, then 1024 strided running sums and a halving tree).

`forced`: an optional list of (power iterations, CG iterations) per outer iteration that replaces the two inner stopping
tests, so that a comparison does not hang on a stop that flips under rounding.  Every outer iteration leaves the record the
device leaves (loss, trace, slot, step, powerIters, cgIters, eval, nComponents) plus the margins of the two stops.

The one deliberate deviation from the reference is the device's: cg ends after 1000 iterations, and when curv is 0 or not
finite (the reference's loop has no working cap)."""
import math

import numpy as np

CG_MAX_ITER = 1000


class SegSum:
    """in-order sums of vals[ptr[k]:ptr[k+1]] for every k: short segments step by step side by side, long ones by cumsum"""
    SHORT = 32

    def __init__(self, ptr):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        lens = np.diff(self.ptr)
        self.m = len(lens)
        self.long = [int(k) for k in np.nonzero(lens > self.SHORT)[0]]
        short = lens <= self.SHORT
        self.steps = []
        for t in range(int(lens[short].max()) if short.any() else 0):
            rows = np.nonzero(short & (lens > t))[0]
            self.steps.append((rows, self.ptr[rows] + t))

    def __call__(self, vals, init=None):
        out = np.zeros(self.m) if init is None else np.array(init, dtype=np.float64)
        for rows, idx in self.steps:
            out[rows] += vals[idx]
        for k in self.long:
            out[k] = np.cumsum(np.concatenate(([out[k]], vals[self.ptr[k]:self.ptr[k + 1]])))[-1]
        return out


def ordered_sum(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def tree_sum(a, blk):
    """the device's two stages: a halving tree per workgroup of `blk` items, then kNarrowBlock = 1024 strided running sums
    over the workgroups' partials and a halving tree"""
    a = np.asarray(a, dtype=np.float64)
    nb = max(1, -(-len(a) // blk))
    A = np.zeros(nb * blk)
    A[:len(a)] = a
    A = A.reshape(nb, blk)
    w = blk
    while w > 1:
        w //= 2
        A = A[:, :w] + A[:, w:2 * w]
    part = A[:, 0]
    T = 1024
    M = np.zeros(-(-nb // T) * T)
    M[:nb] = part
    acc = np.zeros(T)
    for row in M.reshape(-1, T):
        acc = acc + row
    w = T
    while w > 1:
        w //= 2
        acc = acc[:w] + acc[w:2 * w]
    return float(acc[0])


class Data:
    """a CSR matrix with ascending, distinct column ids per row, and its column twin (sample ids ascending)"""

    def __init__(self, indptr, indices, data, n, d):
        self.n, self.d = int(n), int(d)
        self.rptr = np.asarray(indptr, dtype=np.int64)
        self.ridx = np.asarray(indices, dtype=np.int64)
        self.rval = np.asarray(data, dtype=np.float64)
        rows = np.repeat(np.arange(self.n), np.diff(self.rptr))
        order = np.argsort(self.ridx, kind="stable")
        self.crow, self.cval, self.ccol = rows[order], self.rval[order], self.ridx[order]
        self.cptr = np.concatenate(([0], np.cumsum(np.bincount(self.ridx, minlength=self.d)))).astype(np.int64)
        self.rsum, self.csum = SegSum(self.rptr), SegSum(self.cptr)

    def dense(self):
        X = np.zeros((self.n, self.d))
        X[np.repeat(np.arange(self.n), np.diff(self.rptr)), self.ridx] = self.rval
        return X


def kernel_row(X, p, ignoreDiag):
    """K[s] of one basis vector: anova (kernels.nim:22-43) or poly (:67-79), degree 2"""
    t = p[X.ridx] * X.rval
    a1 = X.rsum(t)
    if ignoreDiag:
        return (a1 * a1 - X.rsum(t * t)) / 2.0
    return a1 * a1


def decision_function(X, P, lams, w, intercept, ignoreDiag):
    """model/convex_factorization_machine.nim:63-84"""
    out = X.rsum(w[X.ridx] * X.rval) + intercept
    for s in range(len(lams)):
        out = out + lams[s] * kernel_row(X, P[s], ignoreDiag)
    return out


def check_target(y, task):
    y = np.asarray(y, dtype=np.float64)
    return np.sign(y) if task.startswith("c") else y


class Result:
    pass


def hazan_fit(X, y, starts, *, task="regression", maxComponents=30, ignoreDiag=True, fitLinear=True, fitIntercept=True, maxIter=100,
              eta=1000.0, tol=1e-7, nTol=10, maxIterPower=1000, tolPower=1e-7, optimal=True, summation="order", forced=None, warm=None):
    """starts: callable(outer index, d) -> the power method's start vector (not normalised).  warm: a Result to continue from
    (warmStart = true: P, lams, w, intercept and `it` carry over).  -> Result(P, lams, w, intercept, it, history, converged)"""
    n, d = X.n, X.d

    def vsum(a, blk):
        return ordered_sum(a) if summation == "order" else tree_sum(a, blk)

    y = check_target(y, task)
    if warm is None:
        P, lams, w, intercept, self_it = np.zeros((0, d)), np.zeros(0), np.zeros(d), 0.0, 0
    else:
        P, lams, w, intercept, self_it = warm.P.copy(), warm.lams.copy(), warm.w.copy(), warm.intercept, warm.it
    icpt = fitLinear and fitIntercept
    if fitLinear:
        colsq = np.sqrt(X.csum(X.cval * X.cval))  # norm(X, p=2, axis=0) ...
        colsq = colsq * colsq                      # ... squared (hazan.nim:93-94)
        wz = w.copy()
        if icpt:
            wz = np.append(wz, intercept)
            colsq = np.append(colsq, float(n))
        cn = colsq + 1e-5

    def Zv(v):  # mvmul(X, v, Xp) with the dummy column of ones last (hazan.nim:125,180)
        out = X.rsum(X.rval * v[X.ridx])
        return out + 1.0 * v[d] if icpt else out

    def ZTv(u):  # vmmul(u, X, result); the dummy column's entry is a sum over all samples
        out = X.csum(X.cval * u[X.crow])
        return np.append(out, vsum(u, 32)) if icpt else out

    ypl = X.rsum(X.rval * w[X.ridx]) + intercept
    K = [kernel_row(X, P[s], ignoreDiag) for s in range(len(lams))]
    ypq = np.zeros(n)
    for s in range(len(lams)):
        ypq = ypq + lams[s] * K[s]
    res = y - ypq - ypl
    lossOld = math.sqrt(vsum(res * res, 256)) ** 2 / float(n)
    res0 = lossOld
    history, converged, n_tol = [], False, 0
    for outer in range(maxIter):
        if not optimal and len(lams) >= maxComponents:
            break
        f_power, f_cg = (None, None) if forced is None else forced[outer]
        rec = {}
        # ---- powerMethod (tensor.nim:912-934) on q = X^T (residual o (X p)) (- the diagonal) ----
        p = np.array(starts(outer, d), dtype=np.float64)
        p = p / math.sqrt(ordered_sum(np.abs(p) * np.abs(p)))
        ev, ev_old, it_p, diff, diff_prev = 0.0, 0.0, 0, math.inf, math.inf
        for it in range(maxIterPower):
            Xp = X.rsum(X.rval * p[X.ridx]) * res
            q = X.csum(X.cval * Xp[X.crow])
            if ignoreDiag:
                q = X.csum(-(X.cval * X.cval * res[X.crow] * p[X.ccol]), init=q)
            ev = vsum(p * q, 32)
            p = q / math.sqrt(vsum(q * q, 32))
            it_p = it + 1
            diff_prev, diff = diff, abs(ev - ev_old)
            if (f_power is None and it > 0 and diff < tolPower) or (f_power is not None and it_p >= f_power):
                break
            ev_old = ev
        rec.update(powerIters=it_p, eval=ev, powerDiff=diff, powerDiffPrev=diff_prev)
        # ---- append or replace (hazan.nim:144-153) ----
        s = len(lams)
        if s == maxComponents:
            s = int(np.argmin(lams))  # the first minimum (utils.nim:21-24)
            P[s] = p
            ypq = ypq - lams[s] * K[s]
        else:
            P = np.vstack([P, p])
            lams = np.append(lams, 0.0)
            K.append(np.zeros(n))
        K[s] = kernel_row(X, P[s], ignoreDiag)
        ypq = ypq + lams[s] * K[s]
        res = y - ypq - ypl
        # ---- the step size (hazan.nim:49-56) and the update of lams / yPredQuad (:166-174) ----
        if optimal:
            dd = eta * K[s] - ypq
            nrm = math.sqrt(vsum(dd * dd, 32))
            dot = vsum(dd * res, 32)
            raw = dot / (nrm * nrm) if nrm * nrm != 0.0 else (math.nan if dot == 0.0 or dot != dot else math.copysign(math.inf, dot))
            m = 1e-10 if raw <= 1e-10 else raw  # Nim's max(1e-10, raw): `if y <= x: x else: y`
            step = m if m <= 1.0 else 1.0       # Nim's min(m, 1.0): `if x <= y: x else: y`
        else:
            step = 2.0 / (float(self_it) + 2.0)
        lams = lams * (1 - step)
        ypq = ypq * (1 - step)
        lams[s] += eta * step
        ypq = ypq + eta * step * K[s]
        tot = ordered_sum(lams)
        if tot > eta:
            ypq = ypq * (eta / tot)
            lams = lams * (eta / tot)
        # ---- the linear part (hazan.nim:176-196) ----
        res = y - ypq
        it_cg, cg_tol, n1, n1_prev = 0, 0.0, math.inf, math.inf
        if fitLinear:
            b = ZTv(res)
            cg_tol = 1e-5 * (vsum(np.abs(b[:d]), 32) + (abs(b[d]) if icpt else 0.0))
            x = wz * cn
            r = b / cn
            Ap = ZTv(Zv(x / cn)) / cn
            r = r - Ap
            cp = r.copy()
            dotr = vsum(r * r, 256)
            while it_cg < CG_MAX_ITER and not (f_cg is not None and it_cg >= f_cg):
                Ap = ZTv(Zv(cp / cn)) / cn
                curv = vsum(cp[:d] * Ap[:d], 32) + (cp[d] * Ap[d] if icpt else 0.0)
                if curv == 0.0 or not math.isfinite(curv):
                    break
                alpha = dotr / curv
                x = x + alpha * cp
                r = r - alpha * Ap
                dotr_new = vsum(r * r, 256)
                it_cg += 1
                n1_prev, n1 = n1, vsum(np.abs(r), 256)
                if (f_cg is None and n1 < cg_tol) or (f_cg is not None and it_cg >= f_cg):
                    break
                beta = dotr_new / dotr
                dotr = dotr_new
                cp = cp * beta + r
            wz = x / cn
            w = wz[:d].copy()
            ypl = Zv(wz)
            if icpt:
                intercept = float(wz[d])
        elif fitIntercept:
            intercept = vsum(res, 256) / float(n)
            ypl = np.full(n, intercept)
        res = y - ypq - ypl
        lossNew = math.sqrt(vsum(res * res, 256)) ** 2 / float(n)
        rec.update(loss=lossNew, trace=float(np.sum(np.abs(lams))), slot=s, step=step, cgIters=it_cg, nComponents=len(lams),
                   cgTol=cg_tol, cgNorm=n1, cgNormPrev=n1_prev)
        history.append(rec)
        if lossOld - lossNew < tol:
            n_tol += 1
            if n_tol >= nTol:
                converged = True
                break
        else:
            n_tol = 0
        lossOld = lossNew
        self_it += 1
    out = Result()
    out.P, out.lams, out.w, out.intercept, out.it, out.history, out.converged, out.loss0 = P, lams, w, intercept, self_it, history, converged, res0
    return out


# ---- the brute force of the reference's tests/optimizer/hazan_slow.nim: dense everything, predictions from scratch ----
def _dense_kernel(Xd, p, ignoreDiag):
    a1 = Xd @ p
    return (a1 * a1 - (Xd * Xd) @ (p * p)) / 2.0 if ignoreDiag else a1 * a1


def brute_force_fit(Xd, y, starts, *, maxComponents, ignoreDiag, fitLinear, fitIntercept, maxIter, eta, maxIterPower, optimal):
    """the explicit gradient matrix and a dense power method without a stop, a dense preconditioned CG, yPredQuad and
    yPredLinear recomputed from the parameters whenever they are needed (tol = -inf: no outer stop either)"""
    n, d = Xd.shape
    P, lams, w, intercept = np.zeros((0, d)), np.zeros(0), np.zeros(d), 0.0
    icpt = fitLinear and fitIntercept
    Z = np.hstack([Xd, np.ones((n, 1))]) if icpt else Xd
    ZTZ = Z.T @ Z
    cn = np.append((Xd * Xd).sum(axis=0), float(n))[:Z.shape[1]] + 1e-5 if icpt else (Xd * Xd).sum(axis=0) + 1e-5

    def predict():
        ypq = np.zeros(n)
        for s in range(len(lams)):
            ypq += lams[s] * _dense_kernel(Xd, P[s], ignoreDiag)
        return ypq, Xd @ w + intercept

    for it in range(maxIter):
        if not optimal and len(lams) >= maxComponents:
            break
        ypq, ypl = predict()
        res = y - ypq - ypl
        G = (Xd.T * res) @ Xd
        if ignoreDiag:
            G[np.arange(d), np.arange(d)] -= (Xd * Xd).T @ res
        p = np.array(starts(it, d), dtype=np.float64)
        p /= np.linalg.norm(p)
        for _ in range(maxIterPower):
            q = G @ p
            p = q / np.linalg.norm(q)
        if len(lams) == maxComponents:
            s = int(np.argmin(lams))
            P[s] = p
        else:
            s = len(lams)
            P = np.vstack([P, p])
            lams = np.append(lams, 0.0)
        ypq, ypl = predict()
        res = y - ypq - ypl
        if optimal:
            dd = eta * _dense_kernel(Xd, P[s], ignoreDiag) - ypq
            raw = float(dd @ res) / float(dd @ dd)
            step = min(max(1e-10, raw), 1.0)
        else:
            step = 2.0 / (it + 2.0)
        lams = lams * (1 - step)
        lams[s] += eta * step
        if lams.sum() > eta:
            lams = lams * (eta / lams.sum())
        ypq, _ = predict()
        res = y - ypq
        if fitLinear:
            wz = np.append(w, intercept) if icpt else w.copy()
            b = Z.T @ res
            tol_cg = 1e-5 * np.abs(b).sum()
            x = wz * cn
            r = b / cn - (ZTZ @ (x / cn)) / cn
            cp, dotr = r.copy(), float(r @ r)
            for _ in range(CG_MAX_ITER):
                Ap = (ZTZ @ (cp / cn)) / cn
                curv = float(cp @ Ap)
                if curv == 0.0 or not math.isfinite(curv):
                    break
                alpha = dotr / curv
                x = x + alpha * cp
                r = r - alpha * Ap
                dotr_new = float(r @ r)
                if np.abs(r).sum() < tol_cg:
                    break
                cp = cp * (dotr_new / dotr) + r
                dotr = dotr_new
            wz = x / cn
            w = wz[:d].copy()
            if icpt:
                intercept = float(wz[d])
        elif fitIntercept:
            intercept = float(res.sum()) / n
    out = Result()
    out.P, out.lams, out.w, out.intercept = P, lams, w, intercept
    return out
