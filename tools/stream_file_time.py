"""Time of the device-side writer of the binary stream files on the shape of `bench.py --workload ingest`
(1e6 x 1e5, 32 entries per row): dumpStreamFile end to end and its steps -- the pack kernel and the header's max / min
reduction (HIP events on the stream: the context's timing families "stream_pack", "stream_minmax"), the copies to the host (HIP
events on the copy stream), the file writes and the whole call (host clock; the steps overlap, so they do not add up to it) --
and convertSVMLightFile end to end on the svmlight text of the same matrix (written by dumpSVMLightFile).  One warm-up, then
--reps timed runs of each; one JSON line per leg, appended to profiles/stream_file_time.jsonl (--out).  --label names the build.

--convert-only PATH times nothing but convertSVMLightFile on an existing text file and needs only entry points that every
build of the library has: with NIMFM_HIP_LIB naming an older build's libnimfm_hip.so it measures that build, for the comparison
DESIGN.md section 30 records.

    python tools/stream_file_time.py [--samples 1000000] [--features 100000] [--row 32] [--reps 3] [--dir DIR] [--keep-text PATH]
    NIMFM_HIP_LIB=older/libnimfm_hip.so python tools/stream_file_time.py --convert-only PATH --label parent
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
            "runs": [round(float(x), 3) for x in v]}


def convert_only(a, tmp):
    """convertSVMLightFile through the C ABI alone: nfm_ctx_create and nfm_convert_svmlight are in every build"""
    from nimfm_amd import _capi as capi

    L = C.CDLL(capi.LIB_PATH)
    L.nfm_last_error.restype = C.c_char_p
    L.nfm_ctx_create.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.nfm_convert_svmlight.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    ctx = C.c_void_p()
    assert L.nfm_ctx_create(0, None, C.byref(ctx)) == 0, L.nfm_last_error()
    x, y = os.path.join(tmp, "x.bin"), os.path.join(tmp, "y.bin")
    ms = []
    for rep in range(a.reps + 1):
        for p in (x, y):
            if os.path.exists(p):
                os.remove(p)  # new files every time: giving back the pages of the previous ones is not the converter's work
        t0 = time.perf_counter()
        rc = L.nfm_convert_svmlight(ctx, a.convert_only.encode(), x.encode(), y.encode())
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, L.nfm_last_error()
        if rep:
            ms.append(wall)
    import hashlib
    with open(x, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    return [{"leg": "convertSVMLightFile", "build": a.label, "library": os.path.relpath(capi.LIB_PATH, ROOT), "text_bytes": os.path.getsize(a.convert_only),
             "file_bytes": os.path.getsize(x), "file_sha256": digest, "end_to_end_ms": stat(ms)}]


def full(a, tmp):
    import nimfm_amd as nf
    from nimfm_amd import _capi as capi

    def dump_stats():
        pieces, nbytes = C.c_int64(), C.c_int64()
        copy_ms, sink_ms, total_ms = C.c_double(), C.c_double(), C.c_double()
        capi.check(capi.lib().nfm_dump_stats(C.byref(pieces), C.byref(nbytes), C.byref(copy_ms), C.byref(sink_ms), C.byref(total_ms)))
        return pieces.value, nbytes.value, copy_ms.value, sink_ms.value, total_ms.value

    rng = np.random.default_rng(26)
    ctx = nf.default_context()
    n, d, row = a.samples, a.features, a.row
    nnz = n * row
    indices = (np.arange(row) * (d // row) + rng.integers(0, d // row, size=(n, row))).ravel()  # distinct inside a row (bench.py)
    data = rng.uniform(-1, 1, nnz)
    indptr = np.arange(n + 1, dtype=np.int64) * row
    X = nf.newCSRDataset(data, indices, indptr, n, d)
    X.set_targets(np.sign(rng.standard_normal(n)))
    del indices, data
    text = a.keep_text or os.path.join(tmp, "in.svm")
    nf.dumpSVMLightFile(text, X)
    lines = []
    path = os.path.join(tmp, "dump.bin")
    ctx.timing_enable(True)
    legs = {k: [] for k in ("pack_kernel_ms", "minmax_ms", "copy_to_host_ms", "file_write_ms", "call_ms", "end_to_end_ms")}
    for rep in range(a.reps + 1):
        ctx.timing_reset()
        if os.path.exists(path):
            os.remove(path)
        t0 = time.perf_counter()
        nf.dumpStreamFile(path, X, chunkBytes=a.chunk_bytes)
        wall = (time.perf_counter() - t0) * 1e3
        pieces, nbytes, copy_ms, sink_ms, total_ms = dump_stats()
        if rep == 0:
            continue  # warm-up
        for k, v in zip(legs, (ctx.timing_get("stream_pack")[1], ctx.timing_get("stream_minmax")[1], copy_ms, sink_ms, total_ms, wall)):
            legs[k].append(v)
    ctx.timing_enable(False)
    rec = {"leg": "dumpStreamFile", "build": a.label, "n": n, "d": d, "row": row, "file_bytes": nbytes, "pieces": pieces}
    rec.update({k: stat(v) for k, v in legs.items()})
    # the pack kernel reads 12 bytes per entry and 8 per record and writes the file's body
    rec["pack_gb_per_s"] = round((nbytes + nnz * 12 + n * 8) / np.median(legs["pack_kernel_ms"]) / 1e6, 1)
    lines.append(rec)
    os.remove(path)
    del X
    a.convert_only = text
    lines += convert_only(a, tmp)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--row", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--label", default="device packer")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary folder)")
    ap.add_argument("--keep-text", default=None, help="write the svmlight text of the matrix here and leave it behind")
    ap.add_argument("--convert-only", default=None, metavar="PATH", help="time convertSVMLightFile on this text file and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_file_time.jsonl"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.dir)
    try:
        lines = convert_only(a, tmp) if a.convert_only else full(a, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(a.out, "a") as f:
        for rec in lines:
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
