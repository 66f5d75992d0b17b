"""Device time of the column-major dataset ops on cfg2's shape (1e6 x 1e5, 32 entries per row):
toCSCDataset, toCSRDataset, the CSC slice [n/4, 3n/4), a two-part CSC vstack and hstack, normalize of a CSCDataset on both axes
-- each beside the path it replaces at the parent commit, run once in the same process (to_host(), numpy, an upload), and with
the bytes the leg has to move, so that the rate can be read against the streaming rate tools/membench.hip reports (--membench
names the built binary).  Every device leg makes the result's row twin too (one more transposition): that is part of what a
caller waits for, so it is inside the time.  Then the first fit (newCD, one iteration) on a CSCDataset against a CSRDataset of
the same matrix: the difference is the twin, which the CSC handle already paid for when it was made.  Protocol of
tools/dataset_ops_time.py: one warm-up, mean of five with min and max, wall clock around the call with a stream synchronise, one
JSON line per leg, written to profiles/csc_time.jsonl (--out).

    python tools/csc_time.py [--samples 1000000] [--features 100000] [--row 32] [--membench tools/bin/membench] [--out ...]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import nimfm_amd as nf  # noqa: E402
from dataset_ops_time import once, timed  # noqa: E402


def csc_arrays(rows, cols, vals, d):
    """(indptr, sample ids, values) of the columns: a stable sort by column id is the reference's append order"""
    order = np.argsort(cols, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=d))]).astype(np.int64), rows[order], vals[order]


def host_to_csc(X):
    indptr, indices, data, _ = X.to_host()
    rows = np.repeat(np.arange(X.nSamples), indptr[1:] - indptr[:-1])
    cp, ci, cd = csc_arrays(rows, indices, data, X.nFeatures)
    return nf.newCSRDataset(cd, ci, cp, X.nFeatures, X.nSamples)  # (the parent commit has no column type: X^T by rows)


def host_to_csr(cols):
    """cols: (indptr, ids, values, n, d) of a CSC matrix on the host side of the parent commit's path: its device copy is X^T"""
    Xt, n, d = cols
    indptr, indices, data, _ = Xt.to_host()
    col_of = np.repeat(np.arange(d), indptr[1:] - indptr[:-1])
    rp, rj, rv = csc_arrays(col_of, indices, data, n)
    return nf.newCSRDataset(rv, rj, rp, n, d)


def host_csc_slice(cols, a, b):
    Xt, n, d = cols
    indptr, indices, data, _ = Xt.to_host()
    keep = (indices >= a) & (indices < b)
    col_of = np.repeat(np.arange(d), indptr[1:] - indptr[:-1])
    optr = np.concatenate([[0], np.cumsum(np.bincount(col_of[keep], minlength=d))]).astype(np.int64)
    return nf.newCSRDataset(data[keep], indices[keep] - a, optr, d, b - a)


def host_csc_hstack(A, B):
    (pa, ia, da, _), (pb, ib, db, _) = A[0].to_host(), B[0].to_host()
    return nf.newCSRDataset(np.concatenate([da, db]), np.concatenate([ia, ib]), np.concatenate([pa, pb[1:] + pa[-1]]), A[2] + B[2], A[1])


def host_csc_vstack(A, B):
    (pa, ia, da, _), (pb, ib, db, _) = A[0].to_host(), B[0].to_host()
    d = A[2]
    la, lb = pa[1:] - pa[:-1], pb[1:] - pb[:-1]
    ca, cb = np.repeat(np.arange(d), la), np.repeat(np.arange(d), lb)
    dst_a, dst_b = np.arange(len(da)) + pb[ca], np.arange(len(db)) + pa[cb] + la[cb]
    idx, val = np.empty(len(da) + len(db), dtype=np.int64), np.empty(len(da) + len(db))
    idx[dst_a], idx[dst_b], val[dst_a], val[dst_b] = ia, ib + A[1], da, db
    return nf.newCSRDataset(val, idx, pa + pb, d, A[1] + B[1])


def host_csc_normalize(cols, axis):
    Xt, n, d = cols
    indptr, indices, data, _ = Xt.to_host()
    key = indices if axis == 1 else np.repeat(np.arange(d), indptr[1:] - indptr[:-1])
    nv = np.sqrt(np.bincount(key, weights=data * data, minlength=n if axis == 1 else d))  # (not the in-order sum)
    nv[nv == 0.0] = 1.0
    return nf.newCSRDataset(data / nv[key], indices, indptr, d, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--row", type=int, default=32)
    ap.add_argument("--membench", default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n, d, m = a.samples, a.features, a.row
    ids = np.cumsum(rng.integers(1, max(2, d // m), (n, m)), axis=1) - 1
    y = rng.standard_normal(n)
    X = nf.newCSRDataset(rng.uniform(-1, 1, n * m), np.minimum(ids, d - 1).ravel(), np.arange(n + 1, dtype=np.int64) * m, n, d)
    X.set_targets(y)
    ctx = X.ctx
    Xc = nf.toCSCDataset(X)
    half = n // 2
    A, B = Xc[0:half], Xc[half:2 * half]

    def as_rows_of_t(C):  # the parent commit's stand-in for a CSC matrix on the device: X^T by rows
        cp, ci, cd = C.to_host()
        return nf.newCSRDataset(cd, ci, cp, C.nFeatures, C.nSamples), C.nSamples, C.nFeatures

    hXc, hA, hB = (None, None, None) if a.skip_host else (as_rows_of_t(Xc), as_rows_of_t(A), as_rows_of_t(B))
    E = 12  # bytes per entry: int32 id + float64 value
    nnz = X.nnz
    # one transposition per entry: the major id and the position written (8), the counts (4 read), the radix sort's passes over
    # (id, position) -- 8 bits of the id per pass, 16 bytes read and 16 written -- and the gather (16 read, 12 written)
    t_bytes = lambda bits: nnz * (8 + 4 + 32 * max(1, (bits + 7) // 8) + 28)  # noqa: E731
    bits_d, bits_n = int(np.ceil(np.log2(max(d, 2)))), int(np.ceil(np.log2(max(n, 2))))

    def norm(axis):
        def run():
            Y = nf.toCSCDataset(Xc)  # in place: time it on a fresh copy
            ctx.synchronize()
            t0 = time.perf_counter()
            nf.normalize(Y, axis=axis, norm="l2")
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        run()
        ms = [run() for _ in range(5)]
        return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))

    twin = t_bytes(bits_n)  # every CSC result is followed by the transposition that makes its row twin
    legs = [
        ("toCSCDataset", timed(lambda: nf.toCSCDataset(X), ctx), lambda: host_to_csc(X), t_bytes(bits_d) + twin),
        ("toCSRDataset", timed(lambda: nf.toCSRDataset(Xc), ctx), lambda: host_to_csr(hXc), t_bytes(bits_n)),
        ("CSC slice [n/4, 3n/4)", timed(lambda: Xc[n // 4: 3 * n // 4], ctx), lambda: host_csc_slice(hXc, n // 4, 3 * n // 4),
         nnz * 4 + nnz * E + nnz // 2 * E + twin // 2),
        ("CSC vstack of two halves", timed(lambda: nf.vstack(A, B), ctx), lambda: host_csc_vstack(hA, hB), 2 * E * nnz + twin),
        ("CSC hstack of two halves", timed(lambda: nf.hstack(A, B), ctx), lambda: host_csc_hstack(hA, hB), 2 * E * nnz + twin),
        ("CSC normalize axis 1, l2", norm(1), lambda: host_csc_normalize(hXc, 1), E * nnz + 2 * 8 * nnz + twin),
        ("CSC normalize axis 0, l2", norm(0), lambda: host_csc_normalize(hXc, 0), E * nnz + 2 * 8 * nnz + twin),
    ]
    lines = []
    for name, (mean, lo, hi), host, nbytes in legs:
        lines.append(dict(leg=name, n=n, d=d, row=m, device_ms=round(mean, 3), device_ms_min=round(lo, 3), device_ms_max=round(hi, 3),
                          host_path_ms=None if a.skip_host else round(once(host), 1), bytes=int(nbytes), gb_per_s=round(nbytes / mean / 1e6, 1)))
        print(json.dumps(lines[-1]), flush=True)

    # the first fit: everything a fresh dataset's first iteration builds (the schedule, the caches) is inside
    def first_fit(ds):
        fm = nf.newFactorizationMachine("regression", nComponents=8)
        ctx.synchronize()
        t0 = time.perf_counter()
        nf.newCD(maxIter=1, verbose=0, tol=0).fit(ds, y, fm)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first_fit(nf.toCSRDataset(Xc))  # warm-up: code objects, the allocator
    csr_ms = [first_fit(nf.toCSRDataset(Xc)) for _ in range(3)]
    csc_ms = [first_fit(nf.toCSCDataset(Xc)) for _ in range(3)]
    lines.append(dict(leg="first fit (newCD, one iteration, k = 8)", n=n, d=d, row=m, csr_ms=round(float(np.mean(csr_ms)), 1),
                      csc_ms=round(float(np.mean(csc_ms)), 1), csr_ms_all=[round(v, 1) for v in csr_ms], csc_ms_all=[round(v, 1) for v in csc_ms]))
    print(json.dumps(lines[-1]), flush=True)
    if a.membench:
        out = subprocess.run([a.membench], capture_output=True, text=True, timeout=300).stdout
        rates = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\s*(stream[^\n]*?)\s+[\d.]+ us\s+([\d.]+) GB/s", out, flags=re.M)}
        lines.append({"leg": "tools/membench.hip streaming", "gb_per_s": rates})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
