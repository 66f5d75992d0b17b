"""Device iterations of proximal coordinate descent (newPCD) at the shapes of tools/cd_time.py
(ml100k, ml100k_side, random32; degree 2, squared loss) for three regularisers: L1 and row-wise SquaredL12 (CD's level
schedule) and column-wise SquaredL12, newSquaredL12()'s default (the run schedule).  Prints one JSON line per shape and
regulariser: the depth (levels or runs) and the widest level or run of the P sweep, and the device time per iteration
(nfm_opt_epoch, one captured graph, mean over --epochs after one warm-up).  Writes the lines to profiles/pcd_time.jsonl too
(--out).

    python tools/pcd_time.py [--epochs 10] [--shapes ml100k,ml100k_side,random32] [--out profiles/pcd_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nimfm_amd as nf  # noqa: E402
from nimfm_amd import _capi as capi  # noqa: E402
from cd_time import ml100k, random32, to_csr  # noqa: E402

REGS = {"l1": lambda: nf.newL1(), "squaredl12_row": lambda: nf.newSquaredL12(transpose=False),
        "squaredl12_col": lambda: nf.newSquaredL12()}


def device_time(X, y, n, k, reg, epochs, gamma):
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, scale=0.01)
    fm.init(X)
    pcd = nf.newPCD(verbose=0, alpha0=1e-7, alpha=1e-5, beta=1e-3, gamma=gamma, reg=REGS[reg]())
    depth, widest = pcd.schedule(X, fm)
    h = pcd._handle(fm, X.ctx)
    capi.check(capi.lib().nfm_cd_begin_fit(h, X.h))
    ls, vs = C.c_double(), C.c_double()
    capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))  # warm-up: graph capture
    t0 = time.perf_counter()
    for _ in range(epochs):
        capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))
    ms = (time.perf_counter() - t0) * 1e3 / epochs
    fm._pull()
    return ms, depth, widest, ls.value / n, float((fm.P != 0.0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--shapes", default="ml100k,ml100k_side,random32")
    ap.add_argument("--regs", default=",".join(REGS))
    # gamma * n is the strength; at 1e-4 (newPCD's default) every P of the 0.01-scale start is thresholded to 0 at these
    # shapes, at 1e-7 part of P stays non-zero (p_nonzero in the record)
    ap.add_argument("--gamma", type=float, default=1e-7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_time.jsonl"))
    a = ap.parse_args()
    makers = {"ml100k": lambda: ml100k(False), "ml100k_side": lambda: ml100k(True), "random32": random32}
    lines = []
    for name in a.shapes.split(","):
        rows, n, d, y, k = makers[name]()
        indptr, idx, val = to_csr(rows, n)
        X = nf.newCSRDataset(val, idx, indptr, n, d)
        X.set_targets(y)
        for reg in a.regs.split(","):
            ms, depth, widest, loss, nonzero = device_time(X, y, n, k, reg, a.epochs, a.gamma)
            line = json.dumps({"shape": name, "reg": reg, "gamma": a.gamma, "n": n, "d": d, "nnz": int(len(idx)), "k": k,
                               "schedule": "runs" if reg == "squaredl12_col" else "levels", "depth": depth, "widest": widest,
                               "device_ms_per_iter": round(ms, 4), "mean_loss": loss, "p_nonzero": round(nonzero, 4)})
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
