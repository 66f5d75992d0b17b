"""Times the Ranker on the GPU: newRanker (the two side launches), Ranker.recommend(100) after it, and --
for comparison -- the only way a field-aware model could rank before: hstack(U[rep], V[tile]) of 64 users against every item and
decisionFunction on it, scaled by nU / 64.  Also three ranking calls through one degree-2 Ranker against the three
FactorizationMachine calls they replace.  Host clock around calls that end in a device synchronise (every one copies its
result to the host); each figure is the median of --reps runs after one warm-up, with the least and the most.

    python tools/ranker_time.py --out profiles/ranker_time.jsonl
"""
import argparse
import json
import time

import numpy as np

import nimfm_amd as nf


def timed(fn, reps):
    fn()  # warm-up: code objects, the block cache
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def rows(rng, n, d, per_field, F=0):
    """n rows with per_field entries of every field (F = 0: a plain dataset of per_field entries)"""
    m = per_field * max(F, 1)
    indptr = np.arange(n + 1, dtype=np.int64) * m
    indices = rng.randint(0, d, size=n * m).astype(np.int64)
    data = rng.uniform(-1.0, 1.0, size=n * m)
    if not F:
        return nf.newCSRDataset(data, indices, indptr, n, d)
    return nf.newCSRFieldDataset(data, indices, indptr, np.tile(np.repeat(np.arange(F, dtype=np.int64), per_field), n), n, d, F)


def field_aware(name, nU, nV, FU, FV, dU, dV, k, per_u, per_v, reps):
    rng = np.random.RandomState(1)
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=k)
    ffm.set_params(rng.normal(size=(FU + FV, dU + dV, k)) * 0.1, rng.normal(size=dU + dV) * 0.1, 0.1)
    U, V = rows(rng, nU, dU, per_u, FU), rows(rng, nV, dV, per_v, FV)
    R = nf.newRanker(ffm, U, V)
    n64 = min(64, nU)
    rep, til = np.repeat(np.arange(n64), nV), np.tile(np.arange(nV), n64)

    def pairs():
        return ffm.decisionFunction(nf.hstack(U[rep], V[til]))

    X = nf.hstack(U[rep], V[til])
    got, ref = nf.newRanker(ffm, U[np.arange(n64)], V).scores(), pairs().reshape(n64, nV)  # (a row's bits do not depend on its set)
    rec = {"case": name, "nU": nU, "nV": nV, "FU": FU, "FV": FV, "k": k, "entries_per_user": per_u * FU, "entries_per_item": per_v * FV,
           "worst_rel_diff_to_pairs": float(np.max(np.abs(got - ref) / (1e-12 + np.abs(ref)))),
           "newRanker": timed(lambda: nf.newRanker(ffm, U, V), reps), "recommend_100": timed(lambda: R.recommend(min(100, nV)), reps),
           "pairs_64_users_build_and_decisionFunction": timed(pairs, reps), "pairs_64_users_decisionFunction_alone": timed(lambda: ffm.decisionFunction(X), reps)}
    rec["pairs_all_users_ms_scaled"] = round(rec["pairs_64_users_build_and_decisionFunction"]["median_ms"] * nU / n64, 1)
    return rec


def degree_two(nU, nV, d, k, per, reps):
    rng = np.random.RandomState(2)
    fm = nf.FactorizationMachine("r", nComponents=k)
    fm.set_params(rng.normal(size=(1, k, 2 * d)) * 0.1, rng.normal(size=2 * d) * 0.1, 0.1)
    U, V = rows(rng, nU, d, per), rows(rng, nV, d, per)
    held, seen = rows(rng, nU, nV, 2), rows(rng, nU, nV, 20)

    def three_fm():
        fm.rankOf(U, V, held, seen)
        fm.recommendUnseen(U, V, 100, seen)
        fm.crossDecisionFunctionAt(U, V, held)

    def three_ranker():
        R = nf.newRanker(fm, U, V)
        R.rankOf(held, seen)
        R.recommend(100, seen)
        R.scoresAt(held)

    return {"case": "degree2_three_calls", "nU": nU, "nV": nV, "k": k, "calls": "rankOf + recommend(100, seen) + scoresAt", "fm_methods": timed(three_fm, reps),
            "one_ranker_with_its_creation": timed(three_ranker, reps), "crossDecisionFunction_sides_alone": timed(lambda: nf.newRanker(fm, U, V), reps)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ranker_time.jsonl")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for rec in (field_aware("8x8_fields_k8", 16384, 16384, 8, 8, 20000, 20000, 8, 1, 1, a.reps),
                    field_aware("ml100k_like_4+3_fields_k8", 943, 1682, 4, 3, 1000, 1720, 8, 1, 2, a.reps),
                    degree_two(16384, 16384, 2000, 64, 8, a.reps)):
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
            f.flush()
