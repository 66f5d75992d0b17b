"""Time of the device-side dataset dump on cfg2's shape (1e6 x 1e5, 32 entries per row, values over 16
decades as tests/test_gpu_ingest.py::random_csr_text(wide=True) draws them): dumpSVMLightFile end to end and its steps -- the
length pass, the two scans, the write pass (HIP events on the stream: the context's timing families), the copies to the host
(HIP events on the copy stream), the file writes and the whole call (host clock; the steps overlap, so they do not add up to
it).  Beside them, from the same run: the path it replaces (to_host() + one repr() per entry, written once), the device's own
parse of the same text (nfm_dataset_ingest_stats), and tools/membench.hip's streaming rate when --membench names the built
program, so that the write pass can be read against what the memory system delivers for the bytes it moves.  Then fm.dump of a
--model-features x --model-components model against the Python lines.  Protocol of tools/dataset_ops_time.py: one warm-up, mean
and min-max of five, one JSON line per leg, written to profiles/dataset_dump_time.jsonl (--out).  --label names the build
(the write pass was built in two shapes once: the span staged in LDS, and every lane storing its own bytes).

    python tools/dataset_dump_time.py [--samples 1000000] [--features 100000] [--row 32] [--model-features 1000000]
                                      [--model-components 64] [--membench tools/bin/membench] [--skip-host] [--out ...]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import nimfm_amd as nf  # noqa: E402
from nimfm_amd import _capi as capi  # noqa: E402
from nimfm_amd import host  # noqa: E402


def dump_stats():
    pieces, nbytes = C.c_int64(), C.c_int64()
    copy_ms, sink_ms, total_ms = C.c_double(), C.c_double(), C.c_double()
    capi.check(capi.lib().nfm_dump_stats(C.byref(pieces), C.byref(nbytes), C.byref(copy_ms), C.byref(sink_ms), C.byref(total_ms)))
    return pieces.value, nbytes.value, copy_ms.value, sink_ms.value, total_ms.value


def stat(v):
    return {"mean": round(float(np.mean(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def host_dump(path, X, y):
    """what a caller had before: the arrays on the host, one repr() per number (oracle/ingest.py::dump_svmlight's loop)"""
    indptr, indices, data, _ = X.to_host()
    indptr, indices, data, y = indptr.tolist(), indices.tolist(), data.tolist(), y.tolist()
    with open(path, "w") as f:
        for i in range(len(y)):
            s = repr(y[i])
            for q in range(indptr[i], indptr[i + 1]):
                s += " %d:%s" % (indices[q] + 1, repr(data[q]))
            f.write(s if i == 0 else "\n" + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--row", type=int, default=32)
    ap.add_argument("--model-features", type=int, default=1000000)
    ap.add_argument("--model-components", type=int, default=64)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--membench", default=None)
    ap.add_argument("--skip-host", action="store_true", help="leave out the two Python paths (minutes at the default shapes)")
    ap.add_argument("--label", default="span staged in LDS")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary folder)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_dump_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(24)
    ctx = nf.default_context()
    n, d, row = a.samples, a.features, a.row
    nnz = n * row
    indices = np.sort(rng.integers(0, d, (n, row)), axis=1).ravel()
    data = rng.uniform(-1, 1, nnz) * 10.0 ** rng.integers(-8, 8, nnz)
    indptr = np.arange(n + 1, dtype=np.int64) * row
    y = rng.standard_normal(n)
    X = nf.newCSRDataset(data, indices, indptr, n, d)
    X.set_targets(y)
    del indices, data
    lines = []
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, "dump.svm")
        ctx.timing_enable(True)
        legs = {k: [] for k in ("length_pass_ms", "scans_ms", "write_pass_ms", "copy_to_host_ms", "file_write_ms", "end_to_end_ms")}
        for rep in range(6):
            ctx.timing_reset()
            if os.path.exists(path):
                os.remove(path)  # a new file every time: giving back the pages of the previous one is not the dump's work
            t0 = time.perf_counter()
            nf.dumpSVMLightFile(path, X, chunkBytes=a.chunk_bytes)
            wall = (time.perf_counter() - t0) * 1e3
            pieces, nbytes, copy_ms, sink_ms, _ = dump_stats()
            if rep == 0:
                continue  # warm-up
            for k, v in zip(legs, (ctx.timing_get("dump_len")[1], ctx.timing_get("dump_scan")[1], ctx.timing_get("dump_write")[1], copy_ms,
                                   sink_ms, wall)):
                legs[k].append(v)
        ctx.timing_enable(False)
        rec = {"leg": "dumpSVMLightFile", "build": a.label, "n": n, "d": d, "row": row, "text_bytes": nbytes, "pieces": pieces}
        rec.update({k: stat(v) for k, v in legs.items()})
        # the write pass reads 10 bytes of decimal, 4 of id and 8 of offset per entry and writes the text
        moved = nbytes + nnz * 22 + n * 26
        rec["write_pass_gb_per_s"] = round(moved / np.mean(legs["write_pass_ms"]) / 1e6, 1)
        lines.append(rec)
        # the device's own parse of the same text
        ds, _ = nf.loadSVMLightFile(path)
        b, up, parse = ds.ingest_stats()
        same = np.array_equal(ds.to_host()[2].view(np.uint64), X.to_host()[2].view(np.uint64))
        lines.append({"leg": "loadSVMLightFile of the dumped file", "bytes": b, "upload_ms": round(up, 3), "parse_ms": round(parse, 3),
                      "values_read_back_bit_for_bit": bool(same)})
        del ds
        if not a.skip_host:
            hp = os.path.join(tmp, "host.svm")
            t0 = time.perf_counter()
            host_dump(hp, X, y)
            ms = (time.perf_counter() - t0) * 1e3
            with open(hp, "rb") as f, open(path, "rb") as g:
                equal = f.read() == g.read()
            lines.append({"leg": "to_host() + one repr() per entry (the path replaced), once", "ms": round(ms, 1), "same_bytes": bool(equal)})
            os.remove(hp)
        os.remove(path)
        del X
        # the model dump
        dm, k = a.model_features, a.model_components
        fm = nf.newFactorizationMachine("regression", nComponents=k, warmStart=True)
        fm.set_params(rng.standard_normal((1, k, dm)) * 0.01, rng.standard_normal(dm) * 0.01, 0.5)
        mp = os.path.join(tmp, "model.txt")
        ms = []
        for rep in range(6):
            if os.path.exists(mp):
                os.remove(mp)
            t0 = time.perf_counter()
            fm.dump(mp)
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"leg": "fm.dump, blocks formatted by nfm_format_f64", "build": a.label, "d": dm, "k": k, "file_bytes": os.path.getsize(mp), "ms": stat(ms)}
        P0 = np.ascontiguousarray(fm.P[0])
        fm_ms = []
        for rep in range(6):
            t0 = time.perf_counter()
            nf.formatF64(P0)
            if rep:
                fm_ms.append((time.perf_counter() - t0) * 1e3)
        rec["format_f64_of_P_ms"] = stat(fm_ms)
        lines.append(rec)
        if not a.skip_host:
            with open(mp, "rb") as f:
                dev_bytes = f.read()
            saved = host._DUMP_DEVICE_MIN
            host._DUMP_DEVICE_MIN = 1 << 62
            t0 = time.perf_counter()
            fm.dump(mp)
            ms1 = (time.perf_counter() - t0) * 1e3
            host._DUMP_DEVICE_MIN = saved
            with open(mp, "rb") as f:
                equal = f.read() == dev_bytes
            lines.append({"leg": "fm.dump, the Python lines (the path replaced), once", "d": dm, "k": k, "ms": round(ms1, 1), "same_bytes": bool(equal)})
    if a.membench:
        out = subprocess.run([a.membench], capture_output=True, text=True, timeout=300).stdout
        rates = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\s*(stream[^\n]*?)\s+[\d.]+ us\s+([\d.]+) GB/s", out, flags=re.M)}
        lines.append({"leg": "tools/membench.hip streaming", "gb_per_s": rates})
    with open(a.out, "a") as f:
        for rec in lines:
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
