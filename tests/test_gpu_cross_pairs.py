"""-m gpu: crossDecisionFunctionAt, recommendAmong and rankingScoreAmong (nimfm_amd/csrc/cross.hip) against
the dense calls, by bytes: a pair's score has the bits of crossDecisionFunction(U, V)[i][j]; the lists are the top K of those bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import nimfm_amd as nf
from cross_cases import csr_arrays, make_case
from nimfm_amd import _capi as capi
from test_gpu_cross import dataset, same_bytes, up

pytestmark = pytest.mark.gpu


def pair_rows(nU, nV, seed=5):
    """lengths 0, 1, 15, 16 (unsorted), 17 (one id three times), 33 and every id, cut to nV; one user: all of them in one row"""
    rng = np.random.RandomState(seed + nV)
    pick = lambda m: [int(j) for j in rng.permutation(nV)[:min(m, nV)]]  # noqa: E731
    thrice = pick(14)
    rows = [[], pick(1), sorted(pick(15)), pick(16), thrice[:5] + [thrice[0]] + thrice[5:] + [thrice[0], thrice[0]], sorted(pick(33)), list(range(nV))]
    return rows if nU == 7 else [sum(rows, [])]


def matrix(rows, nV):
    return dataset([[(j, float(n % 2)) for n, j in enumerate(r)] for r in rows], nV)  # the values, zeros too, mean nothing


@functools.lru_cache(maxsize=None)
def world(nU, nV, k=9, fitLower="explicit", tie=None, nan=False):
    case = make_case("pairs", 9000 + nU + nV + k, nU=nU, nV=nV, dU=8, dV=10, k=k, K=1, fitLower=fitLower, fitLinear=fitLower != "augment", tie=tie)
    if nan:
        case["P"][1, case["dU"] + 2] = np.nan  # items that hold feature 2 of V score NaN (test_gpu_cross.py)
    fm, U, V = up(case)
    return case, fm, U, V, fm.crossDecisionFunction(U, V)


@pytest.mark.parametrize("nU,nV", [(nU, nV) for nU in (1, 7) for nV in (1, 17, 70)])
@pytest.mark.parametrize("fitLower", ("explicit", "augment"))
@pytest.mark.parametrize("k", (1, 30, 33, 129))
def test_scores_are_the_dense_bits(k, fitLower, nU, nV):
    _, fm, U, V, scores = world(nU, nV, k, fitLower)
    rows = pair_rows(nU, nV)
    P = matrix(rows, nV)
    got = fm.crossDecisionFunctionAt(U, V, P)
    assert same_bytes(got, scores[np.repeat(np.arange(nU), [len(r) for r in rows]), np.array([j for r in rows for j in r], dtype=np.int64)])
    assert same_bytes(fm.crossDecisionFunctionAt(U, V, P), got)  # a repeated call
    Pc = nf.toCSCDataset(P)  # read through its row twin: the entries in toCSRDataset's order
    indptr, indices, _, _ = nf.toCSRDataset(Pc).to_host()
    assert same_bytes(fm.crossDecisionFunctionAt(U, V, Pc), scores[np.repeat(np.arange(nU), np.diff(indptr)), indices])


def host_top_among(rows, flat, K):
    """the top K of the bits crossDecisionFunctionAt returned (flat, in the rows' order): a repeated id once, (-1, NaN) past the last"""
    ids, sc, at = np.full((len(rows), K), -1, dtype=np.int64), np.full((len(rows), K), np.nan), 0
    for i, r in enumerate(rows):
        cand, first = np.unique(np.array(r, dtype=np.int64), return_index=True)
        s = flat[at + first] if len(r) else np.zeros(0)
        at += len(r)
        nan = np.isnan(s)
        top = np.lexsort((cand, np.where(nan, 0.0, -s), nan))[:K]
        ids[i, :len(top)], sc[i, :len(top)] = cand[top], s[top]
    return ids, sc


def complement(rows, nV):
    return matrix([[int(j) for j in np.setdiff1d(np.arange(nV), r)] for r in rows], nV)


@pytest.mark.parametrize("nU,nV,nan", [(1, 1, False), (1, 70, False), (7, 17, False), (7, 70, False), (7, 70, True), (7, 300, False)])  # 300: K = 256
def test_recommend_among(nU, nV, nan):
    case, fm, U, V, scores = world(nU, nV, tie=40 if nV > 41 else None, nan=nan)
    rows = pair_rows(nU, nV)
    if case["tie"]:
        rows[-1] = rows[-1] + list(case["tie"])[::-1]  # both of the planted tie, the larger id first
    Cm, everything = matrix(rows, nV), matrix([list(range(nV))] * nU, nV)
    flat = fm.crossDecisionFunctionAt(U, V, Cm)
    assert nan == bool(np.isnan(flat).any())
    for K in sorted({1, min(7, nV), min(nV, 256)}):
        ids, sc = fm.recommendAmong(U, V, K, Cm)
        want = host_top_among(rows, flat, K)
        assert same_bytes(ids, want[0]) and same_bytes(sc, want[1]), K
        assert all(same_bytes(a, b) for a, b in zip((ids, sc), fm.recommendUnseen(U, V, K, seen=complement(rows, nV)))), K
        assert all(same_bytes(a, b) for a, b in zip(fm.recommendAmong(U, V, K, everything), fm.recommend(U, V, K))), K
        assert all(same_bytes(a, b) for a, b in zip(fm.recommendAmong(U, V, K, nf.toCSCDataset(Cm)), (ids, sc))), K
    if case["tie"] and not nan:
        a, b = case["tie"]
        top = fm.recommendAmong(U, V, 2, Cm)
        assert list(top[0][-1]) == [a, b] and top[1][-1, 0].tobytes() == top[1][-1, 1].tobytes()


@pytest.mark.parametrize("K", (1, 7, 256))
def test_ranking_score_among(K):
    _, fm, U, V, _ = world(7, 300, tie=40)
    rows, rng = pair_rows(7, 300), np.random.RandomState(K)
    held = matrix([[int(j) for j in rng.permutation(300)[:rng.randint(1, 2 * K + 3)]] if i % 3 else [] for i in range(7)], 300)  # unsorted, distinct
    got = fm.rankingScoreAmong(U, V, held, K, matrix(rows, 300))
    assert got == fm.rankingScore(U, V, held, K, seen=complement(rows, 300)) and got["nUsers"] == 4


def test_refusals():
    _, fm, U, V, _ = world(7, 70)
    L, h, vp = capi.lib(), fm._push(U.ctx), lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok, out, ids = matrix([[0]] * 7, 70), np.zeros(8), np.zeros(7 * 256, dtype=np.int64)
    F = nf.newCSRFieldDataset(*csr_arrays([[(0, 1.0)]] * 7), np.zeros(7, dtype=np.int64), 7, 70, 1)
    fm3 = nf.FactorizationMachine("r", degree=3, nComponents=2)
    fm3.set_params(np.ones((2, 2, 18)), np.zeros(18), 0.0)
    calls = lambda m, X, K: ((lambda: L.nfm_cross_pairs(m, U.h, V.h, X.h, vp(out)), "pairs"),  # noqa: E731
                             (lambda: L.nfm_cross_topk_among(m, U.h, V.h, X.h, K, vp(ids), vp(np.zeros(7 * 256))), "candidates"),
                             (lambda: L.nfm_cross_rank_metrics_among(m, U.h, V.h, X.h, ok.h, K, vp(out)), "candidates"))
    for m, X, K, code, word in ((h, matrix([[0]] * 7, 71), 1, capi.ERR_INVALID, "%s must be nU x nV"),
                                (h, F, 1, capi.ERR_UNSUPPORTED, "field-aware"), (fm3._push(U.ctx), ok, 1, capi.ERR_UNSUPPORTED, "degree 2"),
                                (h, ok, 0, capi.ERR_INVALID, "topK = 0"), (h, ok, 257, capi.ERR_INVALID, "topK = 257")):
        for call, name in calls(m, X, K)[1 if "topK" in word else 0:]:
            assert call() == code and (word % name if "%s" in word else word) in L.nfm_last_error().decode(), (word, name)
