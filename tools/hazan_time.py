"""Device time of Hazan's algorithm for the convex factorization machine (newHazan) at two shapes of
tools/cd_time.py (ml100k, random32): ms per power iteration and per outer iteration, launches per power iteration, and the
algorithmic bytes of one power iteration -- two passes over the values and indices (the rows, then the column twin) plus the
vectors they read and write -- divided by the measured time, next to the streaming-read rate tools/membench.hip measures
(DESIGN.md section 7).  No CPU time is taken: the reference's hazan.nim was not run here.
Prints one JSON line per shape and writes the lines to profiles/hazan_time.jsonl too (--out).

    python tools/hazan_time.py [--outer 3] [--power 200] [--shapes ml100k,random32] [--out profiles/hazan_time.jsonl]
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

LAUNCHES_PER_POWER_ITER = 4  # row pass, column pass, the scalars, the normalisation (cfm.hip: issue_power)
STREAM_READ_GBPS = 6400.0    # tools/membench.hip, streaming read (6 300 - 6 500 GB/s)


def power_bytes(n, d, nnz, ignore_diag):
    """one power iteration: per pass the values (8 B) and the ids (4 B) of every entry and the pointers; the row pass gathers p
    (8 B per entry, counted once per feature: d) and reads the residual, writes Xp; the column pass gathers Xp (n), with
    ignoreDiag the residual (n) again, reads p, writes q; the normalisation reads q and writes p"""
    return 2 * nnz * 12 + 8 * (n + 1) + 8 * (d + 1) + 8 * (d + 2 * n) + 8 * (n + (n if ignore_diag else 0) + 2 * d) + 16 * d


def fit_time(X, y, d, outer, power):
    """ms per outer iteration of three fits: without the linear part at 1 and at `power` power iterations (the two differ only
    in the power iterations: the slope is the time of one), and with the linear part and the intercept at `power`"""
    rng = np.random.default_rng(0)
    out = {}
    for label, p_iters, fit_linear in (("few", 1, False), ("many", power, False), ("full", power, True)):
        cfm = nf.newConvexFactorizationMachine("regression", maxComponents=outer, fitLinear=fit_linear, fitIntercept=fit_linear, ignoreDiag=True)
        opt = nf.newHazan(maxIter=outer, eta=float(np.abs(y).mean() * 10), verbose=0, tol=-1e300, maxIterPower=p_iters, tolPower=0.0)
        opt.fit(X, y, cfm, powerInit=lambda dd: rng.uniform(-1, 1, dd))  # warm-up: the twin, the graphs
        X.ctx.synchronize()
        t0 = time.perf_counter()
        opt.fit(X, y, cfm, powerInit=lambda dd: rng.uniform(-1, 1, dd))
        X.ctx.synchronize()
        out[label] = ((time.perf_counter() - t0) * 1e3 / outer, opt.history)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outer", type=int, default=3)
    ap.add_argument("--power", type=int, default=200)
    ap.add_argument("--shapes", default="ml100k,random32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hazan_time.jsonl"))
    a = ap.parse_args()
    makers = {"ml100k": lambda: ml100k(False), "random32": random32}
    lines = []
    for name in a.shapes.split(","):
        rows, n, d, y, _ = makers[name]()
        indptr, idx, val = to_csr(rows, n)
        X = nf.newCSRDataset(val, idx, indptr, n, d)
        nnz = int(len(idx))
        t = fit_time(X, y, d, a.outer, a.power)
        ms_power = (t["many"][0] - t["few"][0]) / (a.power - 1)
        nb = power_bytes(n, d, nnz, True)
        line = json.dumps({"shape": name, "n": n, "d": d, "nnz": nnz, "outer_iterations": a.outer, "power_iterations": a.power,
                           "ms_per_outer_iteration": round(t["full"][0], 4), "ms_per_outer_iteration_no_linear_part": round(t["many"][0], 4),
                           "ms_per_outer_iteration_no_linear_part_1_power_iter": round(t["few"][0], 4),
                           "ms_per_power_iteration": round(ms_power, 5), "launches_per_power_iteration": LAUNCHES_PER_POWER_ITER,
                           "cg_iterations": [r["cgIters"] for r in t["full"][1]],
                           "power_iteration_bytes": nb, "power_iteration_gbps": round(nb / ms_power / 1e6, 2),
                           "membench_stream_read_gbps": STREAM_READ_GBPS, "cpu_time_taken": False})
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
