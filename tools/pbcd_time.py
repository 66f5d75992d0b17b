"""Device iterations of proximal block coordinate descent (newPBCD) at the shapes of tools/cd_time.py
(ml100k, ml100k_side, random32; degree 2, squared loss) for L21 (CD's level schedule) and SquaredL21, newPBCD's default (the
run schedule); --regs takes l1 and omegacs (the run schedule) too.  Prints one JSON line per shape and regulariser: the depth (levels or runs) and the widest level or run of
the P sweep, and the device time per iteration (nfm_opt_epoch, one captured graph, mean over --epochs after one warm-up).
Writes the lines to profiles/pbcd_time.jsonl too (--out).

    python tools/pbcd_time.py [--epochs 5] [--shapes ml100k,ml100k_side,random32] [--out profiles/pbcd_time.jsonl]
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

REGS = {"l1": lambda: nf.newL1(), "l21": lambda: nf.newL21(), "squaredl21": lambda: nf.newSquaredL21(),
        "omegacs": lambda: nf.newOmegaCS()}


def device_time(X, y, n, k, reg, epochs, gamma):
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, scale=0.01)
    fm.init(X)
    opt = nf.newPBCD(verbose=0, alpha0=1e-7, alpha=1e-5, beta=1e-3, gamma=gamma, reg=REGS[reg]())
    depth, widest = opt.schedule(X, fm)
    h = opt._handle(fm, X.ctx)
    capi.check(capi.lib().nfm_cd_begin_fit(h, X.h))
    ls, vs = C.c_double(), C.c_double()
    capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))  # warm-up: graph capture
    t0 = time.perf_counter()
    for _ in range(epochs):
        capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))
    ms = (time.perf_counter() - t0) * 1e3 / epochs
    fm._pull()
    return ms, depth, widest, ls.value / n, float((fm.P != 0.0).any(axis=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--shapes", default="ml100k,ml100k_side,random32")
    ap.add_argument("--regs", default="l21,squaredl21")
    ap.add_argument("--gamma", type=float, default=1e-4)  # unscaled here (pbcd.nim:154): newPBCD's default
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbcd_time.jsonl"))
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
                               "schedule": "runs" if reg in ("squaredl21", "omegacs") else "levels", "depth": depth,
                               "widest": widest,
                               "device_ms_per_iter": round(ms, 4), "mean_loss": loss, "rows_nonzero": round(nonzero, 4)})
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
