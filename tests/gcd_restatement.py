"""Greedy coordinate descent for the convex factorization machine at refitFully = false, restated from the reference in its
own loop order: optimizer/greedy_cd.nim:76-94 (fitLams), :97-109 (refitDiag), :320-412 (fitZ), :415-500 (fit),
optimizer/fit_linear.nim:5-37 (fitLinearCD, fitInterceptCD), tensor/tensor.nim:912-934 (powerMethod), optimizer/utils.nim:56-75
(objective).  No GPU, no library: numpy only.

Sums along a row or a column are taken entry after entry in storage order, as the reference's loops (and the device's row
pass, column pass and w sweep) take them.  The reductions over nSamples or nFeatures are switchable as in
hazan_restatement: summation="order" adds in index order as the reference does, summation="tree" follows the device's fixed
trees (32 rows or columns per workgroup in a row / column pass, 256 elements in an element-wise one, then 1024 strided running
sums and a halving tree; the intercept step is the 1024 strided sums alone).

`forced`: an optional dict that replaces the discrete decisions a rounding difference can flip, so that a comparison does not
hang on them: forced["power"] is the list of power-iteration counts, one per inner iteration that adds a base, in the order
they happen; forced["inner"] the list of inner-iteration counts per outer iteration; forced["outer"] the number of outer
iterations.  Every outer iteration leaves the record the host leaves (loss, reg, nComponents, objOld, inner: the list of the
inner records) plus the margins of the stops."""
import math

import numpy as np

from hazan_restatement import Result, check_target, kernel_row, ordered_sum, tree_sum

MU = {"squared": 1.0, "squared_hinge": 2.0, "logistic": 0.25, "huber": 1.0}


def loss_value(loss, y, p, param=1.0):
    """loss.nim:18,33,54-59,84-87"""
    if loss == "squared":
        r = y - p
        return 0.5 * (r * r)
    if loss == "squared_hinge":
        z = 1 - p * y
        m = np.where(z > 0, z, 0.0)
        return m * m
    if loss == "logistic":
        z = p * y
        with np.errstate(over="ignore"):
            return np.where(z > 0, np.log(1 + np.exp(-z)), np.log(np.exp(z) + 1) - z)
    z = np.abs(y - p)
    return np.where(z < param, 0.5 * (z * z), param * (z - 0.5 * param))


def loss_grad(loss, y, p, param=1.0):
    """loss.nim:21,36-39,62-67,90-93 (Huber's sign as written)"""
    if loss == "squared":
        return p - y
    if loss == "squared_hinge":
        z = 1 - p * y
        return np.where(z > 0, -2 * y * z, 0.0)
    if loss == "logistic":
        z = p * y
        with np.errstate(over="ignore"):
            return np.where(z > 0, -y * np.exp(-z) / (1 + np.exp(-z)), -y / (np.exp(z) + 1))
    z = np.abs(y - p)
    return np.where(z < param, y - p, param)


def fit_lams(lam, update, norm, beta, mu):
    """greedy_cd.nim:86-94: no guard on invStepSize, the three-way soft threshold as written"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float64(mu) * np.float64(norm)
        lam = np.float64(lam) - np.float64(update) / inv
        if (lam - beta / inv) > 0:
            lam = lam - beta / inv
        elif (lam + beta / inv) < 0:
            lam = lam + beta / inv
        else:
            lam = np.float64(0.0)
    return float(lam)


def gcd_fit(X, y, starts, *, task="regression", loss="squared", lossParam=1.0, maxComponents=30, ignoreDiag=True, fitLinear=True,
            fitIntercept=True, maxIter=10, alpha0=1e-6, alpha=1e-3, beta=1e-5, maxIterInner=10, nRefitting=10, tol=1e-7, maxIterPower=100,
            tolPower=1e-7, summation="order", forced=None, warm=None):
    """starts: callable(draw index, d) -> the power method's start vector (not normalised); the draw index counts the inner
    iterations that add a base, over the whole fit.  warm: a Result to continue from (warmStart = true).
    -> Result(P, lams, w, intercept, history, converged, loss0, reg0, draws)"""
    n, d = X.n, X.d
    tree = summation != "order"
    mu = MU[loss]

    def vsum(a, blk):
        return tree_sum(a, blk) if tree else ordered_sum(a)

    y = check_target(y, task)
    if warm is None:
        P, lams, w, intercept = np.zeros((0, d)), np.zeros(0), np.zeros(d), 0.0
    else:
        P, lams, w, intercept = warm.P.copy(), warm.lams.copy(), warm.w.copy(), warm.intercept
    nd = float(n)
    a0n, an, bn = alpha0 * nd, alpha * nd, beta * nd
    colsq = None
    if fitLinear:
        colsq = np.sqrt(X.csum(X.cval * X.cval))
        colsq = colsq * colsq

    def linear_pred():
        return X.rsum(X.rval * w[X.ridx]) + intercept

    def outer_objective(yp):
        lo = vsum(loss_value(loss, y, yp, lossParam), 256) / nd
        nrm = math.sqrt(vsum(np.abs(w) * np.abs(w), 256))
        reg = 0.5 * alpha0 * (intercept * intercept) + 0.5 * alpha * (nrm * nrm)
        reg += beta * ordered_sum(np.abs(lams))
        return lo, reg

    def inner_objective(yp):
        return (ordered_sum(np.abs(lams)) * bn + vsum(loss_value(loss, y, yp, lossParam), 256)) / nd

    K = [kernel_row(X, P[s], ignoreDiag) for s in range(len(lams))]
    yp = linear_pred()
    for s in range(len(lams)):
        yp = yp + lams[s] * K[s]
    lossOld, regOld = outer_objective(yp)
    loss0, reg0 = lossOld, regOld
    history, converged, draws = [], False, 0
    f_power = None if forced is None else list(forced.get("power", [])) or None
    f_inner = None if forced is None else forced.get("inner")
    f_outer = None if forced is None else forced.get("outer")
    for it in range(maxIter):
        if f_outer is not None and it >= f_outer:
            break
        # ---- fitInterceptCD (fit_linear.nim:28-38) ----
        if fitIntercept:
            dl = loss_grad(loss, y, yp, lossParam)
            if tree:
                u = (a0n * intercept + tree_sum(dl, 1)) / (mu * nd + a0n)
            else:
                u = ordered_sum(np.concatenate(([a0n * intercept], dl))) / (mu * nd + a0n)
            intercept = intercept - u
            yp = yp - u
        # ---- fitLinearCD (fit_linear.nim:5-25): feature after feature, each column in storage order ----
        if fitLinear:
            for j in range(d):
                q0, q1 = X.cptr[j], X.cptr[j + 1]
                if q0 == q1 and w[j] == 0.0:
                    continue  # an empty column at w = 0: the update is an * 0 / inv = 0 and nothing moves
                rows, vals = X.crow[q0:q1], X.cval[q0:q1]
                upd = ordered_sum(np.concatenate(([an * w[j]], loss_grad(loss, y[rows], yp[rows], lossParam) * vals)))
                inv = mu * colsq[j] + an
                if inv < 1e-12:
                    continue
                upd = upd / inv
                w[j] -= upd
                yp[rows] = yp[rows] - upd * vals
        # ---- fitZ (greedy_cd.nim:320-412) ----
        nComponents = int(np.count_nonzero(lams))
        objOld = inner_objective(yp)
        outer = dict(nComponentsStart=nComponents, objOld=objOld, inner=[])
        for itIn in range(maxIterInner):
            if f_inner is not None and itIn >= f_inner[it]:
                break
            rec = dict(it=itIn, added=0, slot=-1, lam=0.0, powerIters=0, eval=0.0)
            if nComponents < maxComponents:
                dL = loss_grad(loss, y, yp, lossParam)
                fp = None if f_power is None else f_power[draws]
                p = np.array(starts(draws, d), dtype=np.float64)
                draws += 1
                p = p / math.sqrt(ordered_sum(np.abs(p) * np.abs(p)))
                ev, ev_old, it_p, diff, diff_prev = 0.0, 0.0, 0, math.inf, math.inf
                for itp in range(maxIterPower):
                    Xp = X.rsum(X.rval * p[X.ridx]) * dL
                    q = X.csum(X.cval * Xp[X.crow])
                    if ignoreDiag:
                        q = X.csum(-(X.cval * X.cval * dL[X.crow] * p[X.ccol]), init=q)
                    ev = vsum(p * q, 32)
                    p = q / math.sqrt(vsum(q * q, 32))
                    it_p = itp + 1
                    diff_prev, diff = diff, abs(ev - ev_old)
                    if (fp is None and itp > 0 and diff < tolPower) or (fp is not None and it_p >= fp):
                        break
                    ev_old = ev
                zeros = np.nonzero(lams == 0.0)[0]
                if len(zeros):
                    s = int(zeros[0])
                    P[s] = p
                else:
                    s = len(lams)
                    lams = np.append(lams, 0.0)
                    P = np.vstack([P, p])
                    K.append(None)
                K[s] = kernel_row(X, P[s], ignoreDiag)
                lams[s] = fit_lams(lams[s], vsum(dL * K[s], 32), vsum(K[s] * K[s], 32), bn, mu)
                if lams[s] != 0.0:
                    yp = yp + lams[s] * K[s]
                    nComponents += 1
                    rec["added"] = 1
                rec.update(slot=s, lam=float(lams[s]), powerIters=it_p, eval=ev, powerDiff=diff, powerDiffPrev=diff_prev)
            refit = (itIn + 1) % nRefitting == 0
            if refit:  # refitDiag (:97-109)
                nComponents = 0
                for s in range(len(lams)):
                    if lams[s] != 0.0:
                        dL = loss_grad(loss, y, yp, lossParam)
                        old = lams[s]
                        lams[s] = fit_lams(old, vsum(dL * K[s], 256), vsum(K[s] * K[s], 256), bn, mu)
                        yp = yp - old * K[s]
                        yp = yp + lams[s] * K[s]
                        if lams[s] != 0.0:
                            nComponents += 1
            rec.update(refit=refit, nComponents=nComponents, nStored=len(lams), objective=inner_objective(yp))
            rec["checked"] = bool(rec["added"]) or refit or itIn == maxIterInner - 1
            outer["inner"].append(rec)
            if rec["checked"]:
                rec["innerDiff"] = abs(rec["objective"] - objOld)
                if f_inner is None and rec["innerDiff"] < tol:
                    break
                objOld = rec["objective"]
        lossNew, regNew = outer_objective(yp)
        outer.update(loss=lossNew, reg=regNew, nComponents=nComponents, lams=lams.copy(), outerDiff=abs(lossNew + regNew - lossOld - regOld))
        history.append(outer)
        if f_outer is None and outer["outerDiff"] < tol:
            converged = True
            break
        lossOld, regOld = lossNew, regNew
        if it < maxIter - 1:
            yp = linear_pred()
            for s in range(len(lams)):
                yp = yp + lams[s] * K[s]
    out = Result()
    out.P, out.lams, out.w, out.intercept, out.history, out.converged = P, lams, w, intercept, history, converged
    out.loss0, out.reg0, out.draws = loss0, reg0, draws
    return out


def counts_of(history):
    """the discrete decisions of a fit, in the shape `forced` takes them"""
    return dict(power=[r["powerIters"] for o in history for r in o["inner"] if r["slot"] >= 0], inner=[len(o["inner"]) for o in history],
                outer=len(history))


# ---- the brute force of the reference's tests/optimizer/greedy_cd_slow.nim at refitFully = false, squared loss: dense
# everything, the explicit gradient matrix, predictions from scratch whenever they are needed ----
def _dense_kernel(Xd, p, ignoreDiag):
    a1 = Xd @ p
    return (a1 * a1 - (Xd * Xd) @ (p * p)) / 2.0 if ignoreDiag else a1 * a1


def brute_force_fit(Xd, y, starts, *, maxComponents, ignoreDiag, fitLinear, fitIntercept, maxIter, alpha0, alpha, beta, maxIterInner,
                    nRefitting, maxIterPower):
    """tol = 0 and tolPower = 0: no stop anywhere (greedy_cd_slow.nim:327,405 compare |.| < 0)"""
    n, d = Xd.shape
    nd = float(n)
    a0n, an, bn = alpha0 * nd, alpha * nd, beta * nd
    P, lams, w, intercept = np.zeros((maxComponents, d)), np.zeros(maxComponents), np.zeros(d), 0.0
    K = np.zeros((maxComponents, n))
    colsq = (Xd * Xd).sum(axis=0)

    def predict():
        return intercept + Xd @ w + (lams[:, None] * K).sum(axis=0)

    def fitlams(s, dL):
        inv = float(K[s] @ K[s])
        lam = lams[s] - float(dL @ K[s]) / inv
        lams[s] = lam - bn / inv if lam - bn / inv > 0 else (lam + bn / inv if lam + bn / inv < 0 else 0.0)

    draws = 0
    yp = predict()
    for it in range(maxIter):
        if fitIntercept:
            u = (a0n * intercept + float((yp - y).sum())) / (nd + a0n)
            intercept -= u
            yp = yp - u
        if fitLinear:
            for j in range(d):
                inv = colsq[j] + an
                if inv < 1e-12:
                    continue
                u = (an * w[j] + float((yp - y) @ Xd[:, j])) / inv
                w[j] -= u
                yp = yp - u * Xd[:, j]
        nc = int(np.count_nonzero(lams))
        for itIn in range(maxIterInner):
            yp = predict()
            if nc < maxComponents:
                dL = yp - y
                G = (Xd.T * dL) @ Xd
                if ignoreDiag:
                    G[np.arange(d), np.arange(d)] -= (Xd * Xd).T @ dL
                    G *= 0.5
                p = np.array(starts(draws, d), dtype=np.float64)
                draws += 1
                p /= np.linalg.norm(p)
                for _ in range(maxIterPower):
                    q = G @ p
                    p = q / np.linalg.norm(q)
                s = int(np.nonzero(lams == 0.0)[0][0])
                P[s] = p
                K[s] = _dense_kernel(Xd, p, ignoreDiag)
                fitlams(s, dL)
                yp = predict()
                if lams[s] != 0.0:
                    nc += 1
            if (itIn + 1) % nRefitting == 0:
                nc = 0
                for s in range(maxComponents):
                    if lams[s] != 0.0:
                        fitlams(s, yp - y)
                        yp = predict()
                        if lams[s] != 0.0:
                            nc += 1
    out = Result()
    out.P, out.lams, out.w, out.intercept = P, lams, w, intercept
    return out
