"""Device time of GreedyCD for the convex factorization machine (newGreedyCD) at the two shapes of
tools/hazan_time.py (ml100k, random32): ms per power iteration (the slope between two maxIterPower values), ms per refitDiag
per non-zero component, ms per outer iteration with and without the linear part.  The power iteration's kernels are Hazan's,
so Hazan's own figure is measured again in the same run, `--repeat` times: its spread is the yardstick for the difference
between the two.  No CPU time is taken: the reference's greedy_cd.nim was not run here.
Prints one JSON line per shape and writes the lines to profiles/gcd_time.jsonl too (--out).

    python tools/gcd_time.py [--components 4] [--power 200] [--repeat 3] [--shapes ml100k,random32] [--out profiles/gcd_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import nimfm_amd as nf  # noqa: E402
from cd_time import ml100k, random32, to_csr  # noqa: E402
from hazan_time import LAUNCHES_PER_POWER_ITER, fit_time as hazan_fit_time  # noqa: E402

# per step (gcd.hip): a new base = dL, the power method's chunks, the slot, the P row, K[s] with fitLams' sums, fitLams, yPred;
# refitDiag per stored component = dL with the sums, fitLams, yPred; an objective = the loss sums and the scalars
LAUNCHES = {"new_base_without_power": 6, "refit_per_component": 3, "inner_objective": 2, "outer_objective": 3, "intercept_step": 1}


def timed_fit(X, y, rng, **kw):
    """ms of the second of two equal fits of one optimizer (the first builds the twin, the levels and the graph) and its history"""
    fit_linear = kw.pop("fitLinear")
    comps = kw.pop("maxComponents")
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=comps, fitLinear=fit_linear, fitIntercept=fit_linear, ignoreDiag=True)
    opt = nf.newGreedyCD(verbose=0, tol=0.0, tolPower=0.0, **kw)
    out = None
    for _ in range(2):
        X.ctx.synchronize()
        t0 = time.perf_counter()
        opt.fit(X, y, cfm, powerInit=lambda dd: rng.uniform(-1, 1, dd))
        X.ctx.synchronize()
        out = ((time.perf_counter() - t0) * 1e3, opt.history)
    return out


def measure(X, y, comps, power):
    rng = np.random.default_rng(0)
    # the power iteration: one outer iteration whose `comps` inner iterations each add a base, at 1 and at `power` iterations
    base = dict(maxComponents=comps, maxIter=1, maxIterInner=comps, nRefitting=comps + 1, fitLinear=False)
    few, h_few = timed_fit(X, y, rng, maxIterPower=1, **base)
    many, h_many = timed_fit(X, y, rng, maxIterPower=power, **base)
    runs = sum(1 for o in h_many for r in o["inner"] if r["slot"] >= 0)
    ms_power = (many - few) / ((power - 1) * runs)
    # refitDiag: two outer iterations on the full basis (the first fills it), 100 inner iterations each, with a refit in every
    # inner iteration and with none; the two fits differ in nothing else
    full = dict(maxComponents=comps, maxIter=3, maxIterInner=100, maxIterPower=1, fitLinear=False)
    with_refit, h_refit = timed_fit(X, y, rng, nRefitting=1, **full)
    no_refit, _ = timed_fit(X, y, rng, nRefitting=101, **full)
    refits = sum(r["nComponents"] for o in h_refit for r in o["inner"] if r["refit"])
    # two outer iterations as a user runs them: the first adds the `comps` bases, the second refits the full basis
    outer = dict(maxComponents=comps, maxIter=2, maxIterInner=comps, nRefitting=comps, maxIterPower=power)
    t_lin, h_lin = timed_fit(X, y, rng, fitLinear=True, **outer)
    t_nolin, _ = timed_fit(X, y, rng, fitLinear=False, **outer)
    return dict(ms_per_power_iteration=ms_power, power_runs=runs, ms_per_refit_per_component=(with_refit - no_refit) / max(refits, 1),
                refit_components=refits, ms_per_outer_iteration=t_lin / 2, ms_per_outer_iteration_no_linear_part=t_nolin / 2,
                ms_new_base_1_power_iter=few / comps, n_components=[o["nComponents"] for o in h_lin])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--power", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="ml100k,random32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcd_time.jsonl"))
    a = ap.parse_args()
    makers = {"ml100k": lambda: ml100k(False), "random32": random32}
    lines = []
    for name in a.shapes.split(","):
        rows, n, d, y, _ = makers[name]()
        indptr, idx, val = to_csr(rows, n)
        X = nf.newCSRDataset(val, idx, indptr, n, d)
        g = [measure(X, y, a.components, a.power) for _ in range(a.repeat)]
        hz = []
        for _ in range(a.repeat):  # Hazan's power iteration, the same way tools/hazan_time.py takes it
            t = hazan_fit_time(X, y, d, 3, a.power)
            hz.append((t["many"][0] - t["few"][0]) / (a.power - 1))
        gp = [m["ms_per_power_iteration"] for m in g]
        line = json.dumps({
            "shape": name, "n": n, "d": d, "nnz": int(len(idx)), "components": a.components, "power_iterations": a.power, "repeat": a.repeat,
            "ms_per_power_iteration": [round(v, 5) for v in gp], "hazan_ms_per_power_iteration": [round(v, 5) for v in hz],
            "hazan_spread_ms": round(max(hz) - min(hz), 5), "gcd_minus_hazan_ms": round(float(np.median(gp) - np.median(hz)), 5),
            "launches_per_power_iteration": LAUNCHES_PER_POWER_ITER,
            "ms_per_refit_per_component": [round(m["ms_per_refit_per_component"], 5) for m in g],
            "ms_per_outer_iteration": [round(m["ms_per_outer_iteration"], 4) for m in g],
            "ms_per_outer_iteration_no_linear_part": [round(m["ms_per_outer_iteration_no_linear_part"], 4) for m in g],
            "ms_new_base_1_power_iter": [round(m["ms_new_base_1_power_iter"], 4) for m in g],
            "n_components_per_outer_iteration": g[0]["n_components"], "launches": LAUNCHES, "cpu_time_taken": False})
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
