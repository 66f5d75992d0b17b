"""Times interactionStats and topInteractions(100) of a FactorizationMachine on the GPU, on parameters
generated here:

    ml100k        d = 2625, k = 30, dense -- against what a user did before: numpy's P.T @ P on the host and the three reductions
    dense_1e5     d = 1e5, k = 30, dense (the host product would be 80 GB: not run)
    sparse_1e5    d = 1e5, k = 30, 5 % of the rows non-zero, each on the five factors of one of six groups

Host clock around calls that end in a device synchronise (both calls copy their result back and wait); each figure is the
median of --reps runs after one warm-up, with the least and the most.  The calls include the upload of the parameters on the
first use only (the model stays on the device); `kernels_ms` are the device-event times of the three launch families of one
call, from the context's timing.  mfma_share: the 2 dn^2 Kq / 2 operations of the upper triangle at the 78.6 TFLOP/s f64
matrix peak over the inter_stats time -- only the dense shapes run every tile.

    python tools/interactions_time.py --out profiles/interactions_time.jsonl
"""
import argparse
import json
import os
import time

import numpy as np

import nimfm_amd as nf

PEAK = 78.6e12  # f64 matrix FLOP/s


def timed(fn, reps):
    fn()  # code objects, the block cache, the upload
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def host_path(P):
    W = P.T @ P
    off = (W != 0) & ~np.eye(len(W), dtype=bool)
    return np.abs(W).sum(), int(np.triu(off, 1).sum()), int(off.any(1).sum())


def shape(name, d, k, rows_frac, groups, reps, with_host):
    rng = np.random.RandomState(3)
    P = rng.standard_normal((1, k, d)) * 0.1
    if rows_frac < 1.0:
        keep = rng.rand(d) < rows_frac
        group = rng.randint(0, groups, d)
        P[0] *= keep[None, :] & (np.arange(k)[:, None] // (k // groups) == group[None, :])
    fm = nf.FactorizationMachine("r", nComponents=k)
    fm.set_params(P, np.zeros(d), 0.0)
    ctx = nf.default_context()
    rec = {"shape": name, "d": d, "k": k, "interactionStats": timed(lambda: fm.interactionStats(), reps),
           "topInteractions100": timed(lambda: fm.topInteractions(100), reps)}
    rec["stats"] = fm.interactionStats()
    ctx.timing_enable(True)
    ctx.timing_reset()
    fm.interactionStats()
    fm.topInteractions(100)
    ctx.synchronize()
    rec["kernels_ms"] = {f: round(ctx.timing_get(f)[1], 3) for f in ("inter_rows", "inter_stats", "inter_topk")}
    ctx.timing_enable(False)
    dn = rec["stats"]["nNonzeroRows"]
    if rows_frac == 1.0 and rec["kernels_ms"]["inter_stats"] > 0:
        rec["mfma_share"] = round(dn * dn * 32.0 / PEAK / (rec["kernels_ms"]["inter_stats"] * 1e-3), 4)  # Kq = 32 for k = 30
    if with_host:
        rec["host_numpy"] = timed(lambda: host_path(P[0]), max(3, reps // 2))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    recs = [shape("ml100k", 2625, 30, 1.0, 1, args.reps, True), shape("dense_1e5", 100000, 30, 1.0, 1, args.reps, False),
            shape("sparse_1e5", 100000, 30, 0.05, 6, args.reps, False)]
    for r in recs:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)


if __name__ == "__main__":
    main()
