"""Device epochs of coordinate descent (newCD) against a single-thread C restatement of the
reference's loop (tools/cd_cpu.c, built here with -O2 -ffp-contract=off), at three shapes:

  ml100k       943 users + 1 682 items one-hot, 100 000 pairs with Zipf-skewed item popularity, k = 4
  ml100k_side  the same with side features (about 24 entries per row): user age (7 bins), gender (2), occupation (21),
               activity (10), 6 history slots of 100; item genres (19, 1-6 per item), year (10), 8 tags of 200
  random32     1e5 x 1e4, 32 random entries per row, k = 8

All: degree 2, squared loss.  Prints per shape the schedule depth and widest level of the P sweep, the device time per
iteration (nfm_opt_epoch, one captured graph, mean over --epochs after one warm-up) and the CPU time per iteration.

    python tools/cd_time.py [--epochs 20] [--shapes ml100k,ml100k_side,random32]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nimfm_amd as nf  # noqa: E402
from nimfm_amd import _capi as capi  # noqa: E402


def ml100k(side, seed=0):
    rng = np.random.default_rng(seed)
    nu, ni, n = 943, 1682, 100000
    pop = 1.0 / np.arange(1, ni + 1) ** 1.1
    keys = set()
    users, items = [], []
    while len(users) < n:
        u = rng.integers(0, nu, 2 * n)
        it = rng.choice(ni, 2 * n, p=pop / pop.sum())
        for a, b in zip(u.tolist(), it.tolist()):
            if (a, b) not in keys:
                keys.add((a, b))
                users.append(a)
                items.append(b)
                if len(users) == n:
                    break
    users, items = np.array(users), np.array(items)
    rows = [[(u, 1.0), (nu + i, 1.0)] for u, i in zip(users, items)]
    d = nu + ni
    if side:
        age = rng.integers(0, 7, nu)
        gender = rng.integers(0, 2, nu)
        occ = rng.integers(0, 21, nu)
        genres = [np.sort(rng.choice(19, rng.integers(1, 7), replace=False)) for _ in range(ni)]
        tags = [rng.choice(200, 8, replace=False) for _ in range(ni)]  # 8 item tags of 200
        hist = [rng.choice(100, 6, replace=False) for _ in range(nu)]  # 6 user-history slots of 100
        base = d
        d += 7 + 2 + 21 + 19
        for r, u, i in zip(rows, users, items):
            r += [(base + age[u], 1.0), (base + 7 + gender[u], 1.0), (base + 9 + occ[u], 1.0)]
            r += [(base + 30 + g, 1.0 / len(genres[i])) for g in genres[i]]
            r += [(d + (i % 10), 1.0), (d + 10 + (u % 10), 1.0)]  # item year and user activity bins
            r += [(d + 20 + t, 0.125) for t in tags[i]] + [(d + 220 + t, 1.0 / 6) for t in hist[u]]
        d += 20 + 200 + 100
    y = rng.integers(1, 6, n).astype(np.float64)
    return rows, n, d, y, 4


def random32(seed=0):
    rng = np.random.default_rng(seed)
    n, d, m = 100000, 10000, 32
    rows = []
    for _ in range(n):
        idx = np.sort(rng.choice(d, m, replace=False))
        rows.append(list(zip(idx.tolist(), rng.uniform(-1, 1, m).tolist())))
    return rows, n, d, rng.standard_normal(n), 8


def to_csr(rows, n):
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([j for r in rows for j, _ in sorted(r)], np.int64)
    val = np.array([v for r in rows for _, v in sorted(r)], np.float64)
    return indptr, idx, val


def cpu_time(indptr, idx, val, y, n, d, k, epochs):
    exe = os.path.join(ROOT, "tools", "bin", "cd_cpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "cd_cpu.c"), "-lm"])
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        np.array([n, d, len(idx), k, epochs], np.int64).tofile(f)
        indptr.tofile(f)
        idx.tofile(f)
        val.tofile(f)
        np.asarray(y, np.float64).tofile(f)
        path = f.name
    try:
        out = subprocess.check_output([exe, path], text=True).split()
    finally:
        os.unlink(path)
    return float(out[0])


def device_time(indptr, idx, val, y, n, d, k, epochs):
    X = nf.newCSRDataset(val, idx, indptr, n, d)
    X.set_targets(y)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, scale=0.01)
    fm.init(X)
    cd = nf.newCD(verbose=0, alpha0=1e-7, alpha=1e-5, beta=1e-3)
    depth, widest = cd.schedule(X, fm)
    h = cd._handle(fm, X.ctx)
    capi.check(capi.lib().nfm_cd_begin_fit(h, X.h))
    ls, vs = C.c_double(), C.c_double()
    capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))  # warm-up: graph capture
    t0 = time.perf_counter()
    for _ in range(epochs):
        capi.check(capi.lib().nfm_opt_epoch(h, X.h, None, 0, n, C.byref(ls), C.byref(vs)))
    ms = (time.perf_counter() - t0) * 1e3 / epochs
    return ms, depth, widest, ls.value / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--shapes", default="ml100k,ml100k_side,random32")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    makers = {"ml100k": lambda: ml100k(False), "ml100k_side": lambda: ml100k(True), "random32": random32}
    for name in a.shapes.split(","):
        rows, n, d, y, k = makers[name]()
        indptr, idx, val = to_csr(rows, n)
        ms, depth, widest, loss = device_time(indptr, idx, val, y, n, d, k, a.epochs)
        cpu = None if a.no_cpu else cpu_time(indptr, idx, val, y, n, d, k, max(2, a.epochs // 4))
        print(json.dumps({"shape": name, "n": n, "d": d, "nnz": int(len(idx)), "k": k, "levels": depth, "widest": widest,
                          "device_ms_per_iter": round(ms, 4), "cpu_ms_per_iter": None if cpu is None else round(cpu, 3),
                          "ratio": None if cpu is None else round(cpu / ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
