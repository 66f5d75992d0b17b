"""Time of `load` of a model dump: the number blocks parsed on the device (nfm_parse_f64) against the
Python lines (host._LOAD_DEVICE_MIN = 1 << 62: what `load` did before, and what the result is measured against).

Models are drawn from a seed and dumped once per shape: FM k = 16, d = 1e5; FM k = 64, d = 1e6 (about 1.4 GB of text); FFM
with 16 fields, d = 1e5, k = 8.  Every leg runs in a child process of its own, under its own time limit, so that its peak
resident set (VmHWM, and the sampled peak of RssAnon: the first counts the mapped file's pages too) is its own: host clock
around `load` after one warm-up load, three repeats of the device leg, three of the Python leg (one, without warm-up, at the
largest shape); per device load the kernel time from the context's timing families "load_index" and "load_parse" and
nfm_parse_stats' upload + copy-back, staging and whole-call times, summed over the load's blocks.  The legs' results are compared by a SHA-256 of P, w, lams and the intercept.  Beside
them the least the hardware allows: the text up and 8 bytes per value down over a 63 GB/s host link, and one pass over the
mapped file at the rate this host copies it.  --sweep: one block of 16 x (n / 16) for n = 2^12 ... 2^22, median of five reads
per leg (parseF64 against the loaders' own lines): where the device leg starts to win is host._LOAD_DEVICE_MIN.  One JSON line
per leg to profiles/model_load_time.jsonl.

    python tools/model_load_time.py [--dir DIR] [--shapes small,north,ffm] [--sweep] [--out profiles/model_load_time.jsonl]
"""
import argparse
import ctypes as C
import hashlib
import json
import mmap
import os
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LINK_GBS = 63.0
SHAPES = {"small": ("fm", 16, 100000, 0), "north": ("fm", 64, 1000000, 0), "ffm": ("ffm", 8, 100000, 16)}


def make(kind, k, d, fields, path):
    import nimfm_amd as nf
    rng = np.random.default_rng(31)
    if kind == "fm":
        fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, warmStart=True)
        fm.set_params(rng.standard_normal((1, k, d)) * 0.01, rng.standard_normal(d) * 0.01, 0.125)
    else:
        fm = nf.newFieldAwareFactorizationMachine("regression", nComponents=k, warmStart=True)
        fm.set_params(rng.standard_normal((fields, d, k)) * 0.01, rng.standard_normal(d) * 0.01, 0.125)
    fm.dump(path)


def digest(fm):
    h = hashlib.sha256()
    for a in (fm.P, fm.w, getattr(fm, "lams", np.zeros(0)), [fm.intercept]):
        h.update(memoryview(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cast("B"))
    return h.hexdigest()


def status_mb(key):
    with open("/proc/self/status") as f:
        for ln in f:
            if ln.startswith(key + ":"):
                return int(ln.split()[1]) / 1024.0
    return 0.0


class AnonPeak(threading.Thread):
    """the peak of RssAnon, sampled every 5 ms: VmHWM also counts the pages of the mapped file, which the kernel may drop"""

    def __init__(self):
        super().__init__(daemon=True)
        self.peak, self.stop = 0.0, False

    def run(self):
        while not self.stop:
            self.peak = max(self.peak, status_mb("RssAnon"))
            time.sleep(0.005)


def leg(path, device, reps, warm):
    """child: -> one JSON line"""
    import nimfm_amd as nf
    from nimfm_amd import _capi as capi
    from nimfm_amd import host
    ctx = nf.default_context()
    per_load = []
    if device:
        real = host.parseF64

        def timed(*a, **kw):
            out = real(*a, **kw)
            copy_ms, stage_ms, total_ms, pieces = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            capi.check(capi.lib().nfm_parse_stats(C.byref(pieces), None, C.byref(copy_ms), C.byref(stage_ms), C.byref(total_ms)))
            cur = per_load[-1]
            cur["calls"] += 1
            cur["pieces"] += pieces.value
            cur["copy_ms"] += copy_ms.value
            cur["stage_ms"] += stage_ms.value
            cur["call_ms"] += total_ms.value
            return out
        host.parseF64 = timed
    else:
        host._LOAD_DEVICE_MIN = 1 << 62
    ms, dig = [], None
    sampler = AnonPeak()
    sampler.start()
    for r in range(warm + reps):
        per_load.append({"calls": 0, "pieces": 0, "copy_ms": 0.0, "stage_ms": 0.0, "call_ms": 0.0})
        if device:
            ctx.timing_enable(True)
            ctx.timing_reset()
        t0 = time.perf_counter()
        fm = nf.load(path, False)
        dt = (time.perf_counter() - t0) * 1e3
        if device:
            per_load[-1]["index_ms"] = ctx.timing_get("load_index")[1]
            per_load[-1]["parse_ms"] = ctx.timing_get("load_parse")[1]
            ctx.timing_enable(False)
        dig = digest(fm)
        del fm
        if r >= warm:
            ms.append(dt)
    sampler.stop = True
    sampler.join()
    # (ru_maxrss would do for the first figure, but Linux hands a child its parent's value across exec)
    rec = {"ms": [round(v, 3) for v in ms], "sha256": dig, "peak_rss_mb": round(status_mb("VmHWM"), 1), "peak_anon_mb": round(sampler.peak, 1)}
    if device:
        for key in ("calls", "pieces", "copy_ms", "stage_ms", "call_ms", "index_ms", "parse_ms"):
            rec[key] = round(float(np.median([p[key] for p in per_load[warm:]])), 3)
    print("LEG " + json.dumps(rec), flush=True)


def copy_rate(path):
    """one pass over the mapped file into a fixed buffer: GB/s of this host (the page cache is warm after the dump)"""
    size = os.path.getsize(path)
    buf = bytearray(64 << 20)
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        view = memoryview(mm)
        t0 = time.perf_counter()
        for o in range(0, size, len(buf)):
            n = min(len(buf), size - o)
            buf[:n] = view[o:o + n]
        dt = time.perf_counter() - t0
        view.release()
        mm.close()
    return size / dt / 1e9


def child(path, device, reps, warm, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "device" if device else "python", "--model", path, "--reps", str(reps),
           "--warm", str(warm)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit, check=True).stdout.decode()
    return json.loads([ln for ln in out.split("\n") if ln.startswith("LEG ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--shapes", default="small,north,ffm")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_load_time.jsonl"))
    ap.add_argument("--leg", default="")
    ap.add_argument("--model", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    a = ap.parse_args()
    if a.leg:
        return leg(a.model, a.leg == "device", a.reps, a.warm)
    recs = []
    for name in [s for s in a.shapes.split(",") if s]:
        kind, k, d, fields = SHAPES[name]
        path = os.path.join(a.dir, "model_load_time_%s.txt" % name)
        make(kind, k, d, fields, path)
        size = os.path.getsize(path)
        values = k * d * max(fields, 1) + d
        big = values > 3e7
        dev = child(path, True, 3, 1, 300)
        py = child(path, False, 1 if big else 3, 0 if big else 1, 600)
        rate = copy_rate(path)
        link_ms = (size + 8 * values) / (LINK_GBS * 1e9) * 1e3
        read_ms = size / (rate * 1e9) * 1e3
        rec = {"shape": name, "kind": kind, "k": k, "d": d, "fields": fields, "file_bytes": size, "values": values, "device": dev,
               "python": py, "same_bytes": dev["sha256"] == py["sha256"],
               "speedup_median": round(float(np.median(py["ms"]) / np.median(dev["ms"])), 2),
               "least_link_ms": round(link_ms, 2), "least_read_ms": round(read_ms, 2), "host_copy_gbs": round(rate, 2),
               "bound_by": "file read" if read_ms > link_ms else "host link"}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        os.remove(path)
    if a.sweep:
        import nimfm_amd as nf
        from nimfm_amd import host
        rng = np.random.default_rng(32)
        for e in range(12, 23):
            n = 1 << e
            text = host._number_lines(rng.standard_normal((16, n // 16)) * 0.01).encode()

            def on_device():
                return host.parseF64(text, 16, n // 16)[0]

            def in_python():  # what the loaders do with a block they read themselves
                P = np.zeros((16, n // 16))
                for s_, line in enumerate(text.decode().split("\n")[:16]):
                    P[s_] = [float(v) for v in line.split(" ") if v][: n // 16]
                return P

            t = {}
            for name, fn in (("device", on_device), ("python", in_python)):
                ref = fn()
                ms = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t0) * 1e3)
                t[name] = round(float(np.median(ms)), 3)
                t[name + "_sha"] = hashlib.sha256(ref.tobytes()).hexdigest()
            rec = {"sweep_values": n, "text_bytes": len(text), "device_ms": t["device"], "python_ms": t["python"],
                   "same_bytes": t["device_sha"] == t["python_sha"]}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
