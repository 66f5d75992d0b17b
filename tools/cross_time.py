"""Time of crossDecisionFunction and recommend against the only route there was before them: one row per
(user, item) pair, hstack(U[rep], V[tile]), then decisionFunction.

    python tools/cross_time.py                       # the ml-100k shape (943 x 1682 one-hot rows, k = 30): pairs, cross, recommend(10)
    python tools/cross_time.py --big                 # 1e5 x 1e5, k = 64: recommend(100) alone, FLOP/s of the tile kernel
    python tools/cross_time.py --legs cross,recommend --users 16384 --items 16384 --k 64 --top 100   # the two kernels at one larger shape
    NIMFM_HIP_LIB=older/libnimfm_hip.so python tools/cross_time.py --legs pairs --label parent
    python tools/cross_time.py --legs recommend,recommend_seen --users 16384 --items 16384 --k 64 --top 100 --seen 100   # the mask's cost
    python tools/cross_time.py --legs old_route,recommend_seen --top 10 --seen ml100k   # scores to the host, filter and sort there

    python tools/cross_time.py --legs among,pairs_at --users 16384 --items 16384 --k 64 --top 10 --cand 100   # given candidates
    python tools/cross_time.py --legs complement_seen,gather_route --users 16384 --items 16384 --k 64 --top 10 --cand 100   # the routes before
    python tools/cross_time.py --legs sample,sample_host --users 16384 --items 16384 --cand 100 --seen 100   # sampleCandidates and the host loop

    python tools/cross_time.py --legs rank_of,ranking_score,rank_old_route --users 16384 --items 16384 --k 64 --top 100 --seen 100   # rankOf

Legs rank_of (rankOf: the rank of two held-out items per user among the unseen items), ranking_score (rankingScore at --top on the
same matrices: the top-K kernel's time) and rank_old_route (every score to the host, the count there); the last two call nothing
newer than rankingScore, so they run beside an older build of the package too.
--cand N: N candidates per user, uniform (legs among, pairs_at: recommendAmong, crossDecisionFunctionAt; complement_seen:
recommendUnseen with the candidates' complement as seen; gather_route: hstack(U[rows], V[cols]), decisionFunction, a host sort).
The last two call nothing newer than recommendUnseen, so the tool runs as it is beside an older build of the package.
--seen N: about N seen items per user, uniform; --seen ml100k: row lengths with ml-100k's spread (20 .. 737, mean 106).

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


FAMILIES = ("cross_side", "cross_scores", "cross_topk", "cross_topk_seen", "cross_merge", "cross_pairs", "cross_rank_among", "cross_rank_of_seen",
            "rank_of_candidates", "rank_of_close")


def held_pairs(nU, nV):
    """two distinct held-out ids per user, ascending: [nU][2]"""
    hi = np.sort(np.random.default_rng(35).integers(0, nV, size=(nU, 2)), axis=1)
    hi[:, 1] = np.where(hi[:, 1] == hi[:, 0], (hi[:, 0] + 1) % nV, hi[:, 1])
    return np.sort(hi, axis=1)


def seen_matrix(a, nU, nV, rng):
    """-> (data, indices, indptr): the seen items of every user, ascending"""
    if a.seen == "ml100k":
        lens = np.clip(np.rint(20 + rng.exponential(86.0, size=nU)), 20, min(737, nV)).astype(np.int64)
    else:
        lens = np.minimum(rng.poisson(float(a.seen), size=nU), nV).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(nV, size=m, replace=False)) for m in lens]) if nU < 20000 else \
        np.sort(rng.integers(0, nV, size=(nU, int(lens.max()))), axis=1)[np.arange(int(lens.max()))[None] < lens[:, None]]  # (repeats: the same to the mask)
    return np.ones(len(indices)), indices.astype(np.int64), indptr


def cross_leg(a, sets, P, w, name):
    import nimfm_amd as nf

    ctx = nf.default_context()
    U, V = (nf.newCSRDataset(data, indices, indptr, len(indptr) - 1, width) for data, indices, indptr, width in sets)
    fm = nf.FactorizationMachine("regression", nComponents=a.k)
    fm.set_params(P, w, 0.25)
    tile = tile_shape()
    Kq = max(4, 2 * (1 << max(0, int(np.ceil(np.log2((a.k + 1) // 2))))))  # one block of the device layout (k <= 128)
    call = (lambda: fm.recommend(U, V, a.top)) if name == "recommend" else (lambda: fm.crossDecisionFunction(U, V))
    if name in ("recommend_seen", "old_route"):
        sd, si, sp = seen_matrix(a, U.nSamples, V.nSamples, np.random.default_rng(33))
        if name == "recommend_seen":
            S = nf.newCSRDataset(sd, si, sp, U.nSamples, V.nSamples)
            call = lambda: fm.recommendUnseen(U, V, a.top, seen=S)
        else:  # the route there was: every score to the host, the seen ones set to -inf, a partial sort per user
            rows = np.repeat(np.arange(U.nSamples), np.diff(sp))

            def call():
                sc = fm.crossDecisionFunction(U, V)
                sc[rows, si] = -np.inf
                top = np.argpartition(-sc, a.top - 1, axis=1)[:, :a.top]
                part = np.take_along_axis(sc, top, axis=1)
                order = np.lexsort((top, -part), axis=1)
                return np.take_along_axis(top, order, axis=1), np.take_along_axis(part, order, axis=1)
    if name in ("rank_of", "ranking_score", "rank_old_route"):  # the sample leg's matrices: --seen ids seen, two held out per user
        nU, nV = U.nSamples, V.nSamples
        sd, si, sp = seen_matrix(a, nU, nV, np.random.default_rng(33))
        hi = held_pairs(nU, nV)
        S = nf.newCSRDataset(sd, si, sp, nU, nV)
        H = nf.newCSRDataset(np.ones(2 * nU), hi.ravel(), 2 * np.arange(nU + 1, dtype=np.int64), nU, nV)
        if name == "rank_of":
            call = lambda: fm.rankOf(U, V, H, seen=S)
        elif name == "ranking_score":
            call = lambda: fm.rankingScore(U, V, H, a.top, seen=S)
        else:  # the route there was: every score to the host, the seen ones set to NaN, a count per held-out item
            rows = np.repeat(np.arange(nU), np.diff(sp))

            def call():
                sc = fm.crossDecisionFunction(U, V)
                sc[rows, si] = np.nan
                thr = np.take_along_axis(sc, hi, axis=1)
                return [(sc > thr[:, c:c + 1]).sum(axis=1) + ((sc == thr[:, c:c + 1]) & (np.arange(nV)[None] < hi[:, c:c + 1])).sum(axis=1) for c in (0, 1)]
    if name in ("among", "pairs_at", "complement_seen", "gather_route"):
        nU, nV = U.nSamples, V.nSamples
        cols = np.sort(np.random.default_rng(34).integers(0, nV, size=(nU, a.cand)), axis=1)  # (a repeat counts once everywhere)
        rows = np.repeat(np.arange(nU), a.cand)
        if name == "complement_seen":
            mask = np.ones((nU, nV), dtype=bool)
            mask[rows, cols.ravel()] = False
            si = np.nonzero(mask)[1]
            S = nf.newCSRDataset(np.ones(len(si)), si, np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64), nU, nV)
            del mask, si
            call = lambda: fm.recommendUnseen(U, V, a.top, seen=S)
        elif name == "gather_route":
            def call():
                sc = fm.decisionFunction(nf.hstack(U[rows], V[cols.ravel()])).reshape(nU, a.cand)
                order = np.lexsort((cols, -sc), axis=1)[:, :a.top]
                return np.take_along_axis(cols, order, axis=1), np.take_along_axis(sc, order, axis=1)
        else:
            Cm = nf.newCSRDataset(np.ones(cols.size), cols.ravel(), np.arange(nU + 1, dtype=np.int64) * a.cand, nU, nV)
            call = (lambda: fm.recommendAmong(U, V, a.top, Cm)) if name == "among" else (lambda: fm.crossDecisionFunctionAt(U, V, Cm))
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
    if name in ("among", "pairs_at", "complement_seen", "gather_route"):
        rec["candidates"] = a.cand
        if name != "pairs_at":
            rec["topK"] = a.top
        if name in ("among", "pairs_at"):  # what the pair kernel gathers: one row of Kq doubles of the item side per pair
            rec["gathered_bytes"] = U.nSamples * a.cand * Kq * 8
            rec["pair_kernel_gather_GBps"] = round(rec["gathered_bytes"] / np.median(fam["cross_pairs"]) / 1e6, 1)
        return rec
    kern = {"recommend": "cross_topk", "recommend_seen": "cross_topk_seen", "ranking_score": "cross_topk_seen", "rank_of": "cross_rank_of_seen"}.get(name, "cross_scores")
    if name != "crossDecisionFunction" and name != "recommend":
        rec["seen"] = a.seen
    flop = 2.0 * U.nSamples * V.nSamples * Kq
    rec["tile_kernel_tflops"] = round(flop / np.median(fam[kern]) / 1e9, 2)
    rec["algorithmic_bytes"] = (U.nSamples + V.nSamples) * a.k * 8
    # what the tiling asks of the caches: every workgroup stages its users' and its items' factors once per tile
    rec["staged_bytes"] = int(np.ceil(U.nSamples / tile["TU"]) * np.ceil(V.nSamples / tile["TV"]) * (tile["TU"] + tile["TV"]) * Kq * 8)
    if name != "crossDecisionFunction":
        rec["topK"] = a.top
    else:
        rec["checksum"] = float(res.sum())  # the pairs leg's, to the rounding of the two sums
    return rec


def sample_leg(a, name):
    """sampleCandidates (leg sample) and the host route it replaces (leg sample_host: to_host, a numpy loop per user, newCSRDataset)
    on the same resident seen / held-out matrices: --seen ids excluded and two held out per user, --cand drawn"""
    import nimfm_amd as nf

    ctx = nf.default_context()
    nU, nV = a.users, a.items
    sd, si, sp = seen_matrix(a, nU, nV, np.random.default_rng(33))
    seen = nf.newCSRDataset(sd, si, sp, nU, nV)
    held = nf.newCSRDataset(np.ones(2 * nU), held_pairs(nU, nV).ravel(), 2 * np.arange(nU + 1, dtype=np.int64), nU, nV)

    def host_route():
        ptr, idx, _, _ = seen.to_host()
        hptr, hidx, _, _ = held.to_host()
        rng, rows = np.random.default_rng(36), []
        for i in range(nU):
            mine, keep = idx[ptr[i]:ptr[i + 1]], hidx[hptr[i]:hptr[i + 1]]
            draw = np.unique(rng.integers(0, nV, size=a.cand + a.cand // 4))
            draw = draw[~np.isin(draw, mine)][:a.cand]  # (a little short now and then: the cost is what is measured)
            rows.append(np.union1d(draw, keep))
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        return nf.newCSRDataset(np.ones(int(lens.sum())), np.concatenate(rows), np.concatenate([[0], np.cumsum(lens)]), nU, nV)

    call = host_route if name == "sample_host" else (lambda: nf.sampleCandidates(seen, a.cand, 36, include=held))
    fams = ("cand_union", "cand_sample")
    ctx.timing_enable(True)
    ms, fam = [], {f: [] for f in fams}
    for r in range(a.reps + 1):
        ctx.timing_reset()
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(wall)
            for f in fams:
                fam[f].append(ctx.timing_get(f)[1])
    ctx.timing_enable(False)
    rec = {"leg": name, "build": a.label, "nU": nU, "nV": nV, "seen": a.seen, "candidates": a.cand, "nnz": int(res.nnz), "end_to_end_ms": stat(ms)}
    rec.update({f + "_ms": stat(v) for f, v in fam.items() if max(v) > 0})
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
    ap.add_argument("--cand", type=int, default=100, help="candidates per user (legs among, pairs_at, complement_seen, gather_route)")
    ap.add_argument("--seen", default="100", help="seen items per user (uniform), or ml100k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_time.jsonl"))
    a = ap.parse_args()
    if a.big:
        a.users, a.items, a.k, a.top = 100000, 100000, 64, 100
    if a.leg is None:  # every leg in a process of its own, under its own time limit
        legs = a.legs.split(",") if a.legs else (["recommend"] if a.big else ["pairs", "cross", "recommend"])
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--users", str(a.users), "--items", str(a.items), "--k", str(a.k),
                   "--top", str(a.top), "--reps", str(a.reps), "--label", a.label, "--out", a.out, "--seen", a.seen, "--cand", str(a.cand)]
            subprocess.run(cmd, check=True, timeout=a.timeout)
        return
    if a.leg in ("sample", "sample_host"):
        rec = sample_leg(a, a.leg)
        print(json.dumps(rec))
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
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
