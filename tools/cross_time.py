"""Time of crossDecisionFunction and recommend against the only route there was before them: one row per
(user, item) pair, hstack(U[rep], V[tile]), then decisionFunction.

    python tools/cross_time.py                       # the ml-100k shape (943 x 1682 one-hot rows, k = 30): pairs, cross, recommend(10)
    python tools/cross_time.py --big                 # 1e5 x 1e5, k = 64: recommend(100) alone, FLOP/s of the tile kernel
    python tools/cross_time.py --legs cross,recommend --users 16384 --items 16384 --k 64 --top 100   # the two kernels at one larger shape
    NIMFM_HIP_LIB=older/libnimfm_hip.so python tools/cross_time.py --legs pairs --label parent

The pairs route goes through the C ABI alone (entry points every build of the library has), so that NIMFM_HIP_LIB can name the
parent commit's library.  One warm-up, then --reps timed runs; wall clock of the whole call, results on the host; kernel time
by the context's timing families.  Every leg runs in a process of its own under its own time limit (--timeout seconds); a leg
that runs out, or fails, ends the tool there.  One JSON line per leg, appended to profiles/cross_time.jsonl (--out)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
            "runs": [round(float(x), 3) for x in v]}


def one_hot_rows(n, extra, rng):
    """row i: column i, and `extra` side features out of 64 further columns"""
    width = n + 64
    cols = np.concatenate([np.arange(n)[:, None], n + rng.integers(0, 64, size=(n, extra))], axis=1)
    data = rng.uniform(0.5, 1.5, size=cols.shape)
    return data.ravel(), cols.ravel().astype(np.int64), np.arange(n + 1, dtype=np.int64) * (1 + extra), width


def tile_shape():
    """the tile as nimfm_amd/csrc/cross.h states it"""
    text = open(os.path.join(ROOT, "nimfm_amd", "csrc", "cross.h")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % v, text).group(1)) for k, v in (("TU", "kCrossTU"), ("TV", "kCrossTV"), ("KS", "kCrossKS"))}


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def pairs_route(a, sets, P, w):
    """the parent's route through the C ABI: select_rows twice, hstack, decisionFunction to the host"""
    from nimfm_amd import _capi as capi

    L = C.CDLL(capi.LIB_PATH)
    L.nfm_last_error.restype = C.c_char_p
    vpt, i64, pp = C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)
    L.nfm_ctx_create.argtypes = [C.c_int32, vpt, pp]
    L.nfm_dataset_create_csr.argtypes = [vpt, i64, i64, vpt, vpt, vpt, vpt, i64, vpt, pp]
    L.nfm_dataset_select_rows.argtypes = [vpt, vpt, i64, pp]
    L.nfm_dataset_hstack.argtypes = [vpt, i64, pp]
    L.nfm_dataset_destroy.argtypes = [vpt]
    L.nfm_model_destroy.argtypes = [vpt]
    L.nfm_ctx_destroy.argtypes = [vpt]
    L.nfm_model_create.argtypes = [vpt, C.POINTER(capi.ModelCfg), pp]
    L.nfm_model_set_params.argtypes = [vpt, vpt, vpt, C.c_double, vpt]
    L.nfm_decision_function.argtypes = [vpt, vpt, vpt]

    def ok(rc):
        assert rc == 0, L.nfm_last_error()

    ctx = C.c_void_p()
    ok(L.nfm_ctx_create(0, None, C.byref(ctx)))
    hs = []
    for data, indices, indptr, width in sets:
        h = C.c_void_p()
        ok(L.nfm_dataset_create_csr(ctx, len(indptr) - 1, width, vp(indptr), vp(indices), vp(data), None, 0, None, C.byref(h)))
        hs.append(h)
    nU, nV = len(sets[0][2]) - 1, len(sets[1][2]) - 1
    d = sets[0][3] + sets[1][3]
    cfg = capi.ModelCfg(capi.KIND_FM, 0, 2, a.k, capi.LOWER["explicit"], 1, 1, 0, d, 0)
    m = C.c_void_p()
    ok(L.nfm_model_create(ctx, C.byref(cfg), C.byref(m)))
    ok(L.nfm_model_set_params(m, vp(P), vp(w), 0.25, None))
    rep, til = np.repeat(np.arange(nU, dtype=np.int64), nV), np.tile(np.arange(nV, dtype=np.int64), nU)
    out = np.empty(nU * nV)
    ms = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        hu, hv, hp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ok(L.nfm_dataset_select_rows(hs[0], vp(rep), len(rep), C.byref(hu)))
        ok(L.nfm_dataset_select_rows(hs[1], vp(til), len(til), C.byref(hv)))
        ok(L.nfm_dataset_hstack((C.c_void_p * 2)(hu, hv), 2, C.byref(hp)))
        ok(L.nfm_decision_function(m, hp, vp(out)))
        wall = (time.perf_counter() - t0) * 1e3
        for h in (hu, hv, hp):
            L.nfm_dataset_destroy(h)
        if r:
            ms.append(wall)
    L.nfm_model_destroy(m)
    for h in hs:
        L.nfm_dataset_destroy(h)
    L.nfm_ctx_destroy(ctx)
    return {"leg": "pairs + decisionFunction", "build": a.label, "library": os.path.basename(capi.LIB_PATH), "nU": nU, "nV": nV, "k": a.k,
            "end_to_end_ms": stat(ms), "checksum": float(out.sum())}


FAMILIES = ("cross_side", "cross_scores", "cross_topk", "cross_merge")


def cross_leg(a, sets, P, w, name):
    import nimfm_amd as nf

    ctx = nf.default_context()
    U, V = (nf.newCSRDataset(data, indices, indptr, len(indptr) - 1, width) for data, indices, indptr, width in sets)
    fm = nf.FactorizationMachine("regression", nComponents=a.k)
    fm.set_params(P, w, 0.25)
    tile = tile_shape()
    Kq = max(4, 2 * (1 << max(0, int(np.ceil(np.log2((a.k + 1) // 2))))))  # one block of the device layout (k <= 128)
    call = (lambda: fm.recommend(U, V, a.top)) if name == "recommend" else (lambda: fm.crossDecisionFunction(U, V))
    ctx.timing_enable(True)
    ms, fam = [], {f: [] for f in FAMILIES}
    for r in range(a.reps + 1):
        ctx.timing_reset()
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(wall)
            for f in FAMILIES:
                fam[f].append(ctx.timing_get(f)[1])
    ctx.timing_enable(False)
    rec = {"leg": name, "build": a.label, "nU": U.nSamples, "nV": V.nSamples, "k": a.k, "Kq": Kq, "tile": tile,
           "tile_routine": "v_mfma_f64_16x16x4_f64", "end_to_end_ms": stat(ms)}
    rec.update({f + "_ms": stat(v) for f, v in fam.items() if max(v) > 0})
    kern = "cross_topk" if name == "recommend" else "cross_scores"
    flop = 2.0 * U.nSamples * V.nSamples * Kq
    rec["tile_kernel_tflops"] = round(flop / np.median(fam[kern]) / 1e9, 2)
    rec["algorithmic_bytes"] = (U.nSamples + V.nSamples) * a.k * 8
    # what the tiling asks of the caches: every workgroup stages its users' and its items' factors once per tile
    rec["staged_bytes"] = int(np.ceil(U.nSamples / tile["TU"]) * np.ceil(V.nSamples / tile["TV"]) * (tile["TU"] + tile["TV"]) * Kq * 8)
    if name == "recommend":
        rec["topK"] = a.top
    else:
        rec["checksum"] = float(res.sum())  # the pairs leg's, to the rounding of the two sums
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--big", action="store_true", help="1e5 x 1e5, k = 64, recommend(100) alone")
    ap.add_argument("--legs", default=None, help="comma-separated: pairs, cross, recommend (default: all three; --big: recommend)")
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the tool starts for every leg)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds a leg may take")
    ap.add_argument("--label", default="head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_time.jsonl"))
    a = ap.parse_args()
    if a.big:
        a.users, a.items, a.k, a.top = 100000, 100000, 64, 100
    if a.leg is None:  # every leg in a process of its own, under its own time limit
        legs = a.legs.split(",") if a.legs else (["recommend"] if a.big else ["pairs", "cross", "recommend"])
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--users", str(a.users), "--items", str(a.items), "--k", str(a.k),
                   "--top", str(a.top), "--reps", str(a.reps), "--label", a.label, "--out", a.out]
            subprocess.run(cmd, check=True, timeout=a.timeout)
        return
    rng = np.random.default_rng(32)
    sets = [one_hot_rows(a.users, 3, rng), one_hot_rows(a.items, 3, rng)]
    d = sets[0][3] + sets[1][3]
    P, w = rng.normal(0.0, 0.1, size=(1, a.k, d)), rng.normal(0.0, 0.1, size=d)
    rec = pairs_route(a, sets, P, w) if a.leg == "pairs" else cross_leg(a, sets, P, w, {"cross": "crossDecisionFunction"}.get(a.leg, a.leg))
    print(json.dumps(rec))
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
