"""Milliseconds per inner iteration and per epoch of the device-resident Katyusha (newKatyusha) with L1
and with column-wise SquaredL12, at tools/pgd_time.py's two generated shapes and the reference's default mini-batch size
(nFeatures * nSamples / nnz), next to MBPSGD's time per mini-batch at the same shape and mini-batch size in the same run.

--via-abi times the BASELINE instead: the same inner loop with L1 stepped from the host through entry points that predate the
resident solver only (predictAllWithGrad on the mini-batch's rows as a dataset of their own, at params and at tilde,
set_params, numpy for the dense updates), over --inner inner iterations.  A line with both figures carries their ratio.

One process; every step runs under its own time limit (--step-limit seconds, SIGALRM) and the tool stops at the first
failure.  Lines are printed and appended to profiles/katyusha_time.jsonl (--out).

    python tools/katyusha_time.py [--shapes ml100k_side,cfg2] [--iters 3] [--via-abi] [--out profiles/katyusha_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nimfm_amd as nf  # noqa: E402
from pgd_time import HYPER, limited, make, model  # noqa: E402

ETA = 0.1


def batch_of(n, d, m):
    B = max((d * n) // (n * m), 1)
    return B, (n - 1) // B + 1


def resident(X, y, k, reg, iters, B, inner):
    regs = {"l1": nf.newL1, "squaredl12": nf.newSquaredL12}
    kw = dict(verbose=0, tol=0.0, reg=regs[reg](), eta=ETA, miniBatchSize=B, shuffle=False, **HYPER)
    nf.newKatyusha(maxIter=1, **kw).fit(X, y, model(k))  # warm-up: plans, buffers
    fm = model(k)
    opt = nf.newKatyusha(maxIter=iters, **kw)
    t0 = time.perf_counter()
    opt.fit(X, y, fm)
    wall = (time.perf_counter() - t0) * 1e3
    return {"ms_per_epoch": wall / iters, "ms_per_inner": wall / (iters * inner), "finite": bool(np.isfinite(fm.P).all())}


def mbpsgd(X, y, k, reg, iters, B, inner):
    regs = {"l1": nf.newL1, "squaredl12": nf.newSquaredL12}
    kw = dict(verbose=0, tol=0.0, reg=regs[reg](), eta0=ETA, miniBatchSize=B, shuffle=False, **HYPER)
    nf.newMBPSGD(maxIter=1, **kw).fit(X, y, model(k))
    t0 = time.perf_counter()
    nf.newMBPSGD(maxIter=iters, **kw).fit(X, y, model(k))
    wall = (time.perf_counter() - t0) * 1e3
    return {"ms_per_minibatch": wall / (iters * inner)}


def via_abi(X, y, k, B, inner, n_inner):
    """katyusha.nim:99-137 with L1, stepped on the host between device calls that predate the resident solver"""
    a0, al, be, ga = HYPER["alpha0"], HYPER["alpha"], HYPER["beta"], HYPER["gamma"]
    indptr, indices, data, _ = X.to_host()
    n, d = X.nSamples, X.nFeatures
    fm = model(k)
    fm.init(X)
    tau2 = 1.0 / (2.0 * B)
    tau1, tau3 = 0.5, 1.0 - 0.5 - tau2
    _, _, g = nf.predictAllWithGrad(X, y, fm)
    gave = (g["P"], g["w"], g["intercept"])
    tilde = (fm.P.transpose(0, 2, 1).copy(), fm.w.copy(), fm.intercept)
    z, yy = tuple(np.copy(v) for v in tilde), tuple(np.copy(v) for v in tilde)
    nxt = [np.zeros_like(tilde[0]), np.zeros_like(tilde[1]), 0.0]
    inv = [1.0 / (1.0 + ETA * s) for s in (be, al, a0)]
    lam = ga * ETA / (1.0 + be * ETA)

    def grad_at(p, Xb, yb):
        fm.set_params(np.ascontiguousarray(p[0].transpose(0, 2, 1)), p[1], float(p[2]))
        _, _, gg = nf.predictAllWithGrad(Xb, yb, fm)
        return gg["P"], gg["w"], gg["intercept"]

    t0 = time.perf_counter()
    for it in range(n_inner):
        rows = (np.arange(B) + it * B) % n
        lens = indptr[rows + 1] - indptr[rows]
        take = np.concatenate([np.arange(indptr[i], indptr[i + 1]) for i in rows])
        Xb = nf.newCSRDataset(data[take], indices[take], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), B, d, ctx=X.ctx)
        x = tuple(tau1 * a + tau2 * b + tau3 * c for a, b, c in zip(z, tilde, yy))
        gx, gt = grad_at(x, Xb, y[rows]), grad_at(tilde, Xb, y[rows])
        g = tuple(a + (b - c) for a, b, c in zip(gave, gx, gt))
        zP = (z[0] - ETA * g[0]) * inv[0]
        zP = np.sign(zP) * np.maximum(np.abs(zP) - lam, 0.0)
        z = (zP, (z[1] - ETA * g[1]) * inv[1], (z[2] - ETA * g[2]) * inv[2])
        yy = tuple(tau3 * a + tau2 * b + tau1 * c for a, b, c in zip(yy, tilde, z))
        nxt = [a + b for a, b in zip(nxt, yy)]
    wall = (time.perf_counter() - t0) * 1e3
    return {"ms_per_inner": wall / n_inner, "inner_timed": n_inner, "ms_per_epoch_extrapolated": wall / n_inner * inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml100k_side,cfg2")
    ap.add_argument("--regs", default="l1,squaredl12")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--inner", type=int, default=8, help="inner iterations the host-stepped baseline is timed over")
    ap.add_argument("--via-abi", action="store_true", help="time only the host-stepped baseline (runs on older library versions too)")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "katyusha_time.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    try:
        for shape in a.shapes.split(","):
            X, y, n, d, m, k = limited(a.step_limit, make, shape)
            B, inner = batch_of(n, d, m)
            base = {"shape": shape, "n": n, "d": d, "per_row": m, "k": k, "batch": B, "inner": inner, "iters": a.iters}
            abi = limited(a.step_limit, via_abi, X, y, k, B, inner, a.inner)
            emit(dict(base, mode="via_abi", solver="katyusha", reg="l1", **abi))
            if a.via_abi:
                continue
            for reg in a.regs.split(","):
                r = limited(a.step_limit, resident, X, y, k, reg, a.iters, B, inner)
                p = limited(a.step_limit, mbpsgd, X, y, k, reg, a.iters, B, inner)
                rec = dict(base, mode="resident", solver="katyusha", reg=reg, **r)
                rec["mbpsgd_ms_per_minibatch"] = p["ms_per_minibatch"]
                rec["inner_over_mbpsgd_minibatch"] = r["ms_per_inner"] / p["ms_per_minibatch"]
                if reg == "l1":
                    rec["via_abi_over_resident"] = abi["ms_per_inner"] / r["ms_per_inner"]
                emit(rec)
    finally:
        if a.out and lines:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
