"""Device epochs of PSGD (newPSGD with newL1() / newL21()) at the ml-100k shape and at the random shape with
32 entries per row of tools/cd_time.py (degree 2, squared loss), for k = 8 and k = 64 and both regularisers -- and, on the same
inputs in the same run, newSGD(mode="sequential") through the one-workgroup kernel (NFM_SEQ_WIN=0: the window kernel off), the
yardstick.  Both paths have one sample in flight: they are latency-bound by construction, and the figure that matters is the
time per sample.  Prints one JSON line per shape, k and solver: ms per epoch (mean, min and max over --epochs epochs after one
warm-up epoch), samples/s, and for PSGD the ratio of its mean to SGD's.  Writes the lines to profiles/psgd_seq_time.jsonl (--out).

    python tools/psgd_seq_time.py [--epochs 3] [--shapes ml100k,random32] [--ks 8,64] [--samples N] [--sgd-kernel pipelined|staged]
                                  [--out profiles/psgd_seq_time.jsonl]

--sgd-kernel staged measures SGD's one-workgroup kernel without its pipelined step (degree-2 models otherwise take it): thread =
factor, everything of a sample staged in LDS once -- the pattern PSGD's kernel follows, so the ratio to it is the cost of PSGD's
added passes alone.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NFM_SEQ_WIN"] = "0"  # newSGD(mode="sequential"): the one-workgroup kernel, not the window over the chip
# --sgd-kernel staged: SGD's one-workgroup kernel without its pipelined step (NFM_SEQ_PIPE=0, read once per process) -- the
# staged kernel with thread = factor, the pattern PSGD's kernel follows: what PSGD's added passes cost on top of it
SGD_KERNEL = "staged" if "staged" in [v for i, v in enumerate(sys.argv) if i and sys.argv[i - 1] == "--sgd-kernel"] else "pipelined"
if SGD_KERNEL == "staged":
    os.environ["NFM_SEQ_PIPE"] = "0"

import numpy as np  # noqa: E402

import nimfm_amd as nf  # noqa: E402
from nimfm_amd import _capi as capi  # noqa: E402
from cd_time import ml100k, random32, to_csr  # noqa: E402

REGS = {"l1": nf.newL1, "l21": nf.newL21}
HYPER = dict(eta0=0.01, alpha0=1e-7, alpha=1e-5, beta=1e-3)


def epochs_ms(opt, X, y, fm, n, epochs, begin_fit):
    """one warm-up epoch, then `epochs` timed ones, each one nfm_opt_epoch call over the first n samples in the dataset's order"""
    fm.init(X)
    X.set_targets(y)
    opt._handle(fm, X.ctx, "sequential")
    capi.check(capi.lib().nfm_opt_set_it(opt._h, 1))
    if begin_fit:
        capi.check(capi.lib().nfm_psgd_begin_fit(opt._h, X.h))
    opt._epoch(X, None, 0, n)
    ms, loss = [], 0.0
    for _ in range(epochs):
        t0 = time.perf_counter()
        loss, _ = opt._epoch(X, None, 0, n)
        ms.append((time.perf_counter() - t0) * 1e3)
    opt._finalize_into(fm)
    return ms, loss / n, float((fm.P == 0.0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--shapes", default="ml100k,random32")
    ap.add_argument("--ks", default="8,64")
    ap.add_argument("--gamma", type=float, default=1e-4)
    ap.add_argument("--sgd-kernel", default="pipelined", choices=("pipelined", "staged"))
    ap.add_argument("--samples", type=int, default=0, help="samples per epoch (0: the whole dataset)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psgd_seq_time.jsonl"))
    a = ap.parse_args()
    makers = {"ml100k": lambda: ml100k(False), "random32": random32}
    lines = []
    for name in a.shapes.split(","):
        rows, n_all, d, y, _ = makers[name]()
        indptr, idx, val = to_csr(rows, n_all)
        X = nf.newCSRDataset(val, idx, indptr, n_all, d)
        y = np.asarray(y, dtype=np.float64)
        n = min(n_all, a.samples) if a.samples > 0 else n_all
        for k in (int(v) for v in a.ks.split(",")):
            def model():
                return nf.newFactorizationMachine("regression", degree=2, nComponents=k, scale=0.01)

            base = {"shape": name, "n": n, "d": d, "entries_per_row": round(len(idx) / n_all, 2), "k": k, "epochs": a.epochs}
            sgd_ms, sgd_loss, _ = epochs_ms(nf.newSGD(verbose=0, mode="sequential", **HYPER), X, y, model(), n, a.epochs, False)
            results = [dict(base, solver="sgd_one_workgroup_" + SGD_KERNEL, mean_loss=sgd_loss)]
            all_ms = [sgd_ms]
            for reg in REGS:
                opt = nf.newPSGD(verbose=0, gamma=a.gamma, reg=REGS[reg](), **HYPER)
                ms, loss, zeros = epochs_ms(opt, X, y, model(), n, a.epochs, True)
                results.append(dict(base, solver="psgd_" + reg, gamma=a.gamma, mean_loss=loss, zeros=round(zeros, 4),
                                    ratio_to_sgd=round(float(np.mean(ms)) / float(np.mean(sgd_ms)), 3)))
                all_ms.append(ms)
            for r, ms in zip(results, all_ms):
                r.update(ms_per_epoch=round(float(np.mean(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                         us_per_sample=round(float(np.mean(ms)) * 1e3 / n, 3), samples_per_s=round(n / (float(np.mean(ms)) * 1e-3)))
                line = json.dumps(r)
                print(line, flush=True)
                lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
