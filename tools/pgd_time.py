"""Milliseconds per iteration of the device-resident proximal gradient solvers (newPGD, newFISTA, newNMAPGD; DESIGN.md section
15) with L1 and with column-wise SquaredL12, at two generated shapes:

    ml100k_side  1e5 x 2703, 24 entries per row, k = 30   (the reference's benchmarks/ml100k/sparse_fm_nmapgd.nim shape)
    cfg2         1e6 x 1e5, 32 entries per row, k = 16

Per run it records the wall time per iteration, the mean trials per iteration, and the share of the time the library's own
event timers put in the gradient (pgd_grad), the trial and reduction kernels (pgd_trial) and the forward pass (pgd_forward);
what is left is the host waiting on the record copies.

--via-abi times the BASELINE instead: plain PGD with L1 through entry points that predate the resident solvers only
(predictAllWithGrad, numpy step and soft threshold, set_params, decisionFunction, the loss summed on the host) -- the same
line search on the same data, so the same trials, with the parameters crossing the host boundary once per trial.  A line
with both figures carries their ratio (via_abi_ms / resident_ms for PGD with L1).

One process; every step runs under its own time limit (--step-limit seconds, SIGALRM) and the tool stops at the first
failure.  Lines are printed and appended to profiles/pgd_time.jsonl (--out).

    python tools/pgd_time.py [--shapes ml100k_side,cfg2] [--iters 5] [--via-abi] [--out profiles/pgd_time.jsonl]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nimfm_amd as nf  # noqa: E402

SHAPES = {"ml100k_side": (100000, 2703, 24, 30), "cfg2": (1000000, 100000, 32, 16)}
HYPER = dict(alpha0=1e-7, alpha=1e-5, beta=1e-5, gamma=1e-5)  # the benchmark's beta = gamma = 1e-5
FAMILIES = ("pgd_grad", "pgd_trial", "pgd_forward")


class StepTimeout(Exception):
    pass


def limited(seconds, fn, *a, **kw):
    def on_alarm(signum, frame):
        raise StepTimeout("step exceeded %d s" % seconds)
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    try:
        return fn(*a, **kw)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def make(shape, seed=0):
    """m distinct columns per row: a random start and a per-row stride coprime to d"""
    n, d, m, k = SHAPES[shape]
    rng = np.random.default_rng(seed)
    start = rng.integers(0, d, n)
    stride = rng.integers(1, d // m, n)  # m * stride < d: no wrap onto an earlier column
    cols = (start[:, None] + stride[:, None] * np.arange(m)[None, :]) % d
    cols.sort(axis=1)
    assert (np.diff(cols, axis=1) > 0).all()
    val = rng.uniform(0.1, 1.0, (n, m))
    y = rng.standard_normal(n)
    X = nf.newCSRDataset(val.ravel(), cols.ravel().astype(np.int64), np.arange(n + 1, dtype=np.int64) * m, n, d)
    return X, y, n, d, m, k


def model(k):
    return nf.newFactorizationMachine("regression", degree=2, nComponents=k, scale=0.01, randomState=1)


def resident(X, y, k, algo, reg, iters):
    new = {"pgd": nf.newPGD, "fista": nf.newFISTA, "nmapgd": nf.newNMAPGD}[algo]
    regs = {"l1": nf.newL1, "squaredl12": nf.newSquaredL12}
    fm = model(k)
    new(maxIter=1, verbose=0, tol=0.0, reg=regs[reg](), **HYPER).fit(X, y, fm)  # warm-up: plan, buffers
    fm = model(k)
    opt = new(maxIter=iters, verbose=0, tol=0.0, reg=regs[reg](), **HYPER)
    X.ctx.timing_enable(True)
    X.ctx.timing_reset()
    t0 = time.perf_counter()
    opt.fit(X, y, fm)
    wall = (time.perf_counter() - t0) * 1e3
    X.ctx.synchronize()
    fam = {f: X.ctx.timing_get(f)[1] for f in FAMILIES}
    X.ctx.timing_enable(False)
    trials = [sum(i["trials"]) for i in opt.iterations]
    out = {"ms_per_iter": wall / iters, "mean_trials": float(np.mean(trials)), "trials": trials}
    for f in FAMILIES:
        out["share_" + f] = fam[f] / wall
    out["share_host_wait"] = max(0.0, 1.0 - sum(fam.values()) / wall)
    return out


def via_abi(X, y, k, iters):
    """plain PGD with L1 (pgd.nim:106-217) stepped on the host between device calls that predate the resident solvers"""
    a0, al, be, ga = HYPER["alpha0"], HYPER["alpha"], HYPER["beta"], HYPER["gamma"]
    rho, sigma = 0.5, 1.0
    fm = model(k)
    fm.init(X)
    n = X.nSamples

    def mean_loss(yp):
        return float((0.5 * (y - yp) ** 2).sum()) / n

    trials_all = []
    nf.predictAllWithGrad(X, y, fm)  # warm-up: the one-batch plan
    t0 = time.perf_counter()
    for _ in range(iters):
        oP, ow, ob = fm.P.transpose(0, 2, 1).copy(), fm.w.copy(), fm.intercept
        yp, _, g = nf.predictAllWithGrad(X, y, fm)
        old_loss = mean_loss(yp)
        dot_old = float((oP * g["P"]).sum() + (ow * g["w"]).sum() + ob * g["intercept"])
        eta, trials = 1.0, 0
        while True:
            P = (oP - eta * g["P"]) / (1.0 + eta * be)
            lam = ga * eta / (1.0 + eta * be)
            P = np.sign(P) * np.maximum(np.abs(P) - lam, 0.0)
            w = (ow - eta * g["w"]) / (1.0 + eta * al)
            b = (ob - eta * g["intercept"]) / (1.0 + eta * a0)
            fm.set_params(np.ascontiguousarray(P.transpose(0, 2, 1)), w, b)
            loss = mean_loss(fm.decisionFunction(X))
            trials += 1
            cond = float((P * g["P"]).sum() + (w * g["w"]).sum() + b * g["intercept"]) - dot_old
            cond += 0.5 * float(((P - oP) ** 2).sum() + ((w - ow) ** 2).sum() + (b - ob) ** 2) / eta
            if loss - old_loss <= sigma * cond or eta < 1e-12:
                break
            eta *= rho
        trials_all.append(trials)
    wall = (time.perf_counter() - t0) * 1e3
    return {"ms_per_iter": wall / iters, "mean_trials": float(np.mean(trials_all)), "trials": trials_all}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml100k_side,cfg2")
    ap.add_argument("--algos", default="pgd,fista,nmapgd")
    ap.add_argument("--regs", default="l1,squaredl12")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--via-abi", action="store_true", help="time only the host-stepped baseline (runs on older library versions too)")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgd_time.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    try:
        for shape in a.shapes.split(","):
            X, y, n, d, m, k = limited(a.step_limit, make, shape)
            base = {"shape": shape, "n": n, "d": d, "per_row": m, "k": k, "iters": a.iters}
            abi = limited(a.step_limit, via_abi, X, y, k, a.iters)
            emit(dict(base, mode="via_abi", algo="pgd", reg="l1", **abi))
            if a.via_abi:
                continue
            for algo in a.algos.split(","):
                for reg in a.regs.split(","):
                    r = limited(a.step_limit, resident, X, y, k, algo, reg, a.iters)
                    rec = dict(base, mode="resident", algo=algo, reg=reg, **r)
                    if algo == "pgd" and reg == "l1":
                        rec["via_abi_over_resident"] = abi["ms_per_iter"] / r["ms_per_iter"]
                        rec["same_trials_as_via_abi"] = abi["trials"] == r["trials"]
                    emit(rec)
    finally:
        if a.out and lines:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
