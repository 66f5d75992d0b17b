"""Times the sparse x dense products of a resident dataset on the GPU: mvmul, vmmul and both matmuls at
r = m = 16 and 64, on a 1e6 x 1e5 matrix of 32 entries per row and on the ml-100k shape (943 x 1682, 100000 entries), both
generated here.  Three figures per call:

    device_form   nfm_dataset_*_device on torch tensors: the kernels alone (the call ends in a synchronise)
    host_form     matmul / mvmul / vmmul of the package on numpy arrays: with the upload of the operand and the copy back
    host_path     what a user did before: to_host() and the same sums in numpy (reduceat over rows, bincount over columns)

Host clock around calls that end in a device synchronise; each figure is the median of --reps runs after one warm-up, with
the least and the most (host_path: --host-reps runs, no warm-up -- it is seconds long).  roofline: the bytes the product must
move once (S: 12 per entry + indptr; the dense operand; the result) at 8 TB/s over the device form's median.  The column
calls are timed on the CSRDataset (its column structure made per call) and on toCSCDataset of it.

    python tools/extmath_time.py --out profiles/extmath_time.jsonl
"""
import argparse
import json
import os
import time

import numpy as np
import torch  # before the library, as in bench.py: one HIP runtime in the process

import nimfm_amd as nf
from nimfm_amd import _capi as capi

PEAK = 8e12  # bytes / s


def timed(fn, reps, warm=True):
    if warm:
        fn()  # code objects, the block cache
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def host_path(X, call, D):
    """to_host() and the reference's sums in numpy, one dense column (or row) at a time"""
    indptr, idx, val, _ = X.to_host()
    starts, row = indptr[:-1], np.repeat(np.arange(X.nSamples), np.diff(indptr))
    if call == "mvmul":
        return np.add.reduceat(val * D[idx], starts)
    if call == "vmmul":
        return np.bincount(idx, weights=val * D[row], minlength=X.nFeatures)
    if call == "sd":
        return np.stack([np.add.reduceat(val * D[idx, c], starts) for c in range(D.shape[1])], 1)
    return np.stack([np.bincount(idx, weights=val * D[a, row], minlength=X.nFeatures) for a in range(D.shape[0])])


def shape(name, n, d, per_row, nnz, reps, host_reps):
    rng = np.random.RandomState(5)
    if per_row:
        indptr = np.arange(n + 1, dtype=np.int64) * per_row
    else:  # nnz entries dealt to the rows, every row at least one (reduceat above wants no empty row)
        indptr = np.concatenate([[0], np.cumsum(1 + np.bincount(rng.randint(0, n, nnz - n), minlength=n))]).astype(np.int64)
    indices, data = rng.randint(0, d, size=indptr[-1]).astype(np.int64), rng.uniform(-1.0, 1.0, size=indptr[-1])
    X = nf.newCSRDataset(data, indices, indptr, n, d)
    Xc = nf.toCSCDataset(X)
    L, dev = capi.lib(), torch.device("cuda", 0)
    for call, r in (("mvmul", 1), ("vmmul", 1), ("sd", 16), ("sd", 64), ("ds", 16), ("ds", 64)):
        by_rows = call in ("mvmul", "sd")
        D = rng.normal(size=(d, r) if by_rows else (r, n))
        vec = D[:, 0] if call == "mvmul" else D[0]
        arg = vec if call in ("mvmul", "vmmul") else D  # what the numpy path multiplies by
        Dt = torch.from_numpy(D).to(dev)
        out = torch.empty((n, r) if by_rows else (r, d), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        entry = {"mvmul": lambda S: L.nfm_dataset_mvmul_device(S.h, Dt.data_ptr(), d, out.data_ptr()),
                 "vmmul": lambda S: L.nfm_dataset_vmmul_device(S.h, Dt.data_ptr(), n, out.data_ptr()),
                 "sd": lambda S: L.nfm_dataset_matmul_sd_device(S.h, Dt.data_ptr(), d, r, out.data_ptr()),
                 "ds": lambda S: L.nfm_dataset_matmul_ds_device(S.h, Dt.data_ptr(), r, n, out.data_ptr())}[call]
        host = {"mvmul": lambda S: nf.mvmul(S, vec), "vmmul": lambda S: nf.vmmul(vec, S), "sd": lambda S: nf.matmul(S, D),
                "ds": lambda S: nf.matmul(D, S)}[call]
        capi.check(entry(X))
        want = host_path(X, call, arg)
        got = out.cpu().numpy().reshape(want.shape)
        moved = 12 * X.nnz + 8 * (n + 1 if by_rows else d + 1) + D.nbytes + out.numel() * 8
        rec = {"shape": name, "n": n, "d": d, "nnz": int(X.nnz), "call": call, "r": r, "algorithmic_bytes": int(moved),
               "worst_abs_diff_to_host_path": float(np.max(np.abs(got - want))),
               "device_form": timed(lambda: capi.check(entry(X)), reps), "host_form": timed(lambda: host(X), reps),
               "host_path": timed(lambda: host_path(X, call, arg), host_reps, warm=False)}
        if not by_rows:
            rec["device_form_csc"], rec["host_form_csc"] = timed(lambda: capi.check(entry(Xc)), reps), timed(lambda: host(Xc), reps)
        best = rec["device_form_csc" if not by_rows else "device_form"]["median_ms"]
        rec["roofline_fraction"] = round(moved / PEAK / (best * 1e-3), 4)
        yield rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/extmath_time.jsonl")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--small-only", action="store_true", help="the ml-100k shape alone")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    shapes = [("ml100k", 943, 1682, 0, 100000)] + ([] if a.small_only else [("1e6x1e5x32", 1000000, 100000, 32, 0)])
    with open(a.out, "w") as f:
        for s in shapes:
            for rec in shape(*s, a.reps, a.host_reps):
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                f.flush()
