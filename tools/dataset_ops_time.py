"""Device time of the dataset ops on cfg2's shape (1e6 x 1e5, 32 entries per row): a random 80 %
selection, a contiguous slice, a two-part vstack, a two-part hstack, normalize on both axes -- each beside the path it replaces
in the same run (to_host() + numpy + newCSRDataset) and with the bytes the leg has to move, so that the rate can be read against
the streaming rate tools/membench.hip reports.  Then the rating-file loader on a file of --rating-lines
lines: end to end and parse alone.  Protocol of tools/pbcd_time.py: one warm-up, mean of five, one JSON line per leg, written to
profiles/dataset_ops_time.jsonl (--out).  The host path is run once per leg (it takes seconds).

    python tools/dataset_ops_time.py [--samples 1000000] [--features 100000] [--row 32] [--rating-lines 10000000] [--out ...]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import nimfm_amd as nf  # noqa: E402


def timed(fn, ctx, reps=5):
    fn()  # warm-up
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))


def once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_select(X, rows):
    indptr, indices, data, _ = X.to_host()
    lens = (indptr[1:] - indptr[:-1])[rows]
    optr = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(indptr[rows] - optr[:-1], lens) + np.arange(optr[-1])
    return nf.newCSRDataset(data[src], indices[src], optr, len(rows), X.nFeatures)


def host_vstack(A, B):
    (pa, ia, da, _), (pb, ib, db, _) = A.to_host(), B.to_host()
    return nf.newCSRDataset(np.concatenate([da, db]), np.concatenate([ia, ib]), np.concatenate([pa, pb[1:] + pa[-1]]),
                            A.nSamples + B.nSamples, A.nFeatures)


def host_hstack(A, B):
    (pa, ia, da, _), (pb, ib, db, _) = A.to_host(), B.to_host()
    la, lb = pa[1:] - pa[:-1], pb[1:] - pb[:-1]
    optr = pa + pb
    ra, rb = np.repeat(np.arange(A.nSamples), la), np.repeat(np.arange(B.nSamples), lb)
    dst_a, dst_b = np.arange(len(da)) + pb[ra], np.arange(len(db)) + pa[rb] + la[rb]
    idx, val = np.empty(len(da) + len(db), dtype=np.int64), np.empty(len(da) + len(db))
    idx[dst_a], idx[dst_b], val[dst_a], val[dst_b] = ia, ib + A.nFeatures, da, db
    return nf.newCSRDataset(val, idx, optr, A.nSamples, A.nFeatures + B.nFeatures)


def host_normalize(X, axis):
    indptr, indices, data, _ = X.to_host()
    key = np.repeat(np.arange(X.nSamples), indptr[1:] - indptr[:-1]) if axis == 1 else indices
    nv = np.sqrt(np.bincount(key, weights=data * data, minlength=X.nSamples if axis == 1 else X.nFeatures))  # (not the in-order sum)
    nv[nv == 0.0] = 1.0
    return nf.newCSRDataset(data / nv[key], indices, indptr, X.nSamples, X.nFeatures)


def rating_file(path, n, rng):
    """n lines `uuuuuu::iiiii::r` (zero-padded ids: 16 bytes per line), written from one byte array"""
    users, items, stars = rng.integers(1, 1000000, n), rng.integers(1, 100000, n), rng.integers(1, 6, n)
    buf = np.full((n, 16), ord(":"), dtype=np.uint8)
    for k in range(6):
        buf[:, 5 - k] = 48 + (users // 10**k) % 10
    for k in range(5):
        buf[:, 12 - k] = 48 + (items // 10**k) % 10
    buf[:, 15] = 10
    buf[:, 14] = 48 + stars
    buf.tofile(path)
    return 16 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--row", type=int, default=32)
    ap.add_argument("--rating-lines", type=int, default=10000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_ops_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n, d, m = a.samples, a.features, a.row
    # rows of m distinct ids in ascending order, as cfg2's: a device-made dataset is checked for repeats like any other
    ids = np.cumsum(rng.integers(1, max(2, d // m), (n, m)), axis=1) - 1
    X = nf.newCSRDataset(rng.uniform(-1, 1, n * m), np.minimum(ids, d - 1).ravel(), np.arange(n + 1, dtype=np.int64) * m, n, d)
    ctx = X.ctx
    rows = rng.permutation(n)[: int(0.8 * n)].astype(np.int64)
    half = n // 2
    A, B = X[0:half], X[half:2 * half]
    E = 12  # bytes per entry: int32 id + float64 value
    nnz, ptr = X.nnz, 8 * (n + 1)

    def norm(axis):
        def run():
            Y = X[0:n]  # normalize works in place: time it on a fresh slice, whose own cost is the slice leg's
            t0 = time.perf_counter()
            nf.normalize(Y, axis=axis, norm="l2")
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        run()
        ms = [run() for _ in range(5)]
        return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))

    legs = [
        # name, device (mean, min, max), host path once, bytes read + written
        ("select 80 % at random", timed(lambda: X[rows], ctx), lambda: host_select(X, rows), 2 * E * len(rows) * m + 4 * 8 * len(rows)),
        ("slice [n/4, 3n/4)", timed(lambda: X[n // 4: 3 * n // 4], ctx), lambda: host_select(X, np.arange(n // 4, 3 * n // 4)), E * nnz + ptr),
        ("vstack of two halves", timed(lambda: nf.vstack(A, B), ctx), lambda: host_vstack(A, B), 2 * E * (A.nnz + B.nnz) + 2 * ptr),
        ("hstack of two halves", timed(lambda: nf.hstack(A, B), ctx), lambda: host_hstack(A, B), 2 * E * (A.nnz + B.nnz) + 6 * ptr // 2),
        ("normalize axis 1, l2", norm(1), lambda: host_normalize(X, 1), E * nnz + 2 * 8 * nnz + 2 * ptr),
        ("normalize axis 0, l2", norm(0), lambda: host_normalize(X, 0), E * nnz + 2 * 8 * nnz + 2 * ptr),
    ]
    lines = []
    for name, (mean, lo, hi), host, nbytes in legs:
        lines.append(dict(leg=name, n=n, d=d, row=m, device_ms=round(mean, 3), device_ms_min=round(lo, 3), device_ms_max=round(hi, 3),
                          host_path_ms=round(once(host), 1), bytes=int(nbytes), gb_per_s=round(nbytes / mean / 1e6, 1)))
        print(json.dumps(lines[-1]), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ratings.txt")
        nbytes = rating_file(path, a.rating_lines, rng)
        nf.loadUserItemRatingFile(path)  # warm-up (and the page cache)
        wall, parse, upload = [], [], []
        for _ in range(5):
            t0 = time.perf_counter()
            R, _ = nf.loadUserItemRatingFile(path)
            wall.append((time.perf_counter() - t0) * 1e3)
            _, up, pa = R.ingest_stats()
            upload.append(up)
            parse.append(pa)
        lines.append(dict(leg="loadUserItemRatingFile", lines=a.rating_lines, bytes=nbytes, end_to_end_ms=round(float(np.mean(wall)), 2),
                          upload_ms=round(float(np.mean(upload)), 2), parse_ms=round(float(np.mean(parse)), 2),
                          parse_gb_per_s=round(nbytes / float(np.mean(parse)) / 1e6, 1), shape=R.shape))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
