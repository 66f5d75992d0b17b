"""-m gpu: recommendUnseen, exactly the top K of crossDecisionFunction's bits without the seen pairs, and rankingScore at the
relative bound (K + nE + 4) 2^-52, that many roundings of non-negative terms at the most (cross.hip)."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import nimfm_amd as nf
from cross_cases import csr_arrays, make_case, tile_shape
from nimfm_amd import _capi as capi
from test_gpu_cross import dataset, same_bytes, up

pytestmark = pytest.mark.gpu
T = tile_shape()
TU, TV = T["TU"], T["TV"]
SHAPES = [(nU, nV, K) for nU in (1, TU + 1) for nV in (TV - 1, 2 * TV + 3, 300) for K in (1, 7, min(nV, T["maxTopK"]))]  # K = nV, and 256 of 300


@functools.lru_cache(maxsize=None)
def world(nU, nV):
    case = make_case("seen", 7000 + nU + nV, nU=nU, nV=nV, dU=8, dV=10, k=9, K=7, tie=40)
    fm, U, V = up(case)
    return case, fm, U, V, fm.crossDecisionFunction(U, V)


def seen_rows(case, scores, K):
    """every pattern in a user of its own; the last user (alone in the last, partial user tile) sees the first of the planted tie"""
    nU, nV = scores.shape
    rng = np.random.RandomState(nV + K)
    edges = [j for j in (0, TV - 1, TV, 2 * TV - 1, nV - 1) if j < nV]
    tile0 = TV if nV >= 2 * TV else 0
    repeat = [3] + [5] * 70 + [9, min(TV + 1, nV - 1)]  # 70 copies of one id: more than one round of a window
    patterns = [
        edges, list(range(tile0, min(tile0 + TV, nV))), list(range(nV)),
        [int(j) for j in np.setdiff1d(np.arange(nV), rng.choice(nV, max(K - 2, 0), replace=False))],  # K - 2 candidates are left
        [], [int(j) for j in rng.permutation(nV)[:nV // 3]], repeat,  # an empty row, an unsorted one, the repeats
    ]
    rows = [patterns[i % 8] if i % 8 < 7 else [int(np.nanargmax(scores[i]))] for i in range(nU)]  # i % 8 == 7: the best item
    rows[-1] = [case["tie"][0]] if nU > 1 else edges[::-1] + repeat + [int(np.nanargmax(scores[0]))]
    return rows


def seen_dataset(rows, nV):
    return dataset([[(j, 0.0 if n % 2 else 1.0) for n, j in enumerate(r)] for r in rows], nV)  # an explicit 0 counts too


def host_top_unseen(scores, rows, K):
    ids = np.full((scores.shape[0], K), -1, dtype=np.int64)
    sc = np.full((scores.shape[0], K), np.nan)
    for i, row in enumerate(scores):
        keep = np.setdiff1d(np.arange(len(row)), rows[i])
        nan = np.isnan(row[keep])
        top = keep[np.lexsort((keep, np.where(nan, 0.0, -row[keep]), nan))][:K]
        ids[i, :len(top)], sc[i, :len(top)] = top, row[top]
    return ids, sc


@pytest.mark.parametrize("nU,nV,K", SHAPES)
def test_recommend_unseen_is_the_sorted_unseen_scores(nU, nV, K):
    case, fm, U, V, scores = world(nU, nV)
    rows = seen_rows(case, scores, K)
    S = seen_dataset(rows, nV)
    want_ids, want_scores = host_top_unseen(scores, rows, K)
    for chunk in (0, 1, TV, nV - 1):  # chunk edges cut the seen rows
        ids, sc = fm.recommendUnseen(U, V, K, seen=S, chunkItems=chunk)
        assert same_bytes(ids, want_ids) and same_bytes(sc, want_scores), chunk
    again = fm.recommendUnseen(U, V, K, seen=S)
    assert same_bytes(again[0], ids) and same_bytes(again[1], sc)  # (chunkItems = nV - 1 and 0 agree, and so do two calls)
    got = fm.recommendUnseen(U, V, K, seen=nf.toCSCDataset(S))  # read through its row twin
    assert same_bytes(got[0], ids) and same_bytes(got[1], sc)


def test_no_seen_is_recommend():
    case, fm, U, V, scores = world(TU + 1, 2 * TV + 3)
    assert all(same_bytes(a, b) for a, b in zip(fm.recommendUnseen(U, V, 7, seen=None, chunkItems=TV), fm.recommend(U, V, 7, TV)))


def restated(ids, held, K):
    """precision, recall, hitRate in fractions, ndcg by math.fsum and math.log2, over the users with a held-out item"""
    disc = [1.0 / math.log2(r + 2) for r in range(K)]
    P, R, H, N, n = Fraction(0), Fraction(0), Fraction(0), [], 0
    for row, t in zip(ids, held):
        if t:
            hits = [r for r, j in enumerate(row) if j >= 0 and j in t]
            n += 1
            P, R, H = P + Fraction(len(hits), K), R + Fraction(len(hits), len(t)), H + (1 if hits else 0)
            N.append(Fraction(math.fsum(disc[r] for r in hits)) / Fraction(math.fsum(disc[:min(K, len(t))])))
    mean = lambda x: float(x / n) if n else math.nan  # noqa: E731
    return {"precision": mean(P), "recall": mean(R), "ndcg": mean(sum(N)), "hitRate": mean(H), "nUsers": n}


@pytest.mark.parametrize("K", (1, 7, 256))
@pytest.mark.parametrize("masked", (True, False))
@pytest.mark.parametrize("eligible", (True, False))
def test_ranking_score(K, masked, eligible):
    case, fm, U, V, scores = world(TU + 1, 300)
    nU, nV = scores.shape
    rows = seen_rows(case, scores, K)
    S = seen_dataset(rows, nV) if masked else None
    rng = np.random.RandomState(K)
    held = [[int(j) for j in rng.permutation(nV)[:nV if i == 1 else rng.randint(1, 2 * K + 3)]] if eligible and i % 5 else [] for i in range(nU)]  # unsorted, distinct
    H = dataset([[(j, 1.0) for j in t] for t in held], nV)
    ids, _ = fm.recommendUnseen(U, V, K, seen=S)
    got, want = fm.rankingScore(U, V, H, K, seen=S, chunkItems=TV), restated(ids, [set(t) for t in held], K)
    assert got["nUsers"] == want["nUsers"] == (sum(1 for t in held if t))
    bound = (K + want["nUsers"] + 4) * 2.0 ** -52
    for name in ("precision", "recall", "ndcg", "hitRate"):
        assert abs(got[name] - want[name]) <= bound * abs(want[name]) if eligible else math.isnan(got[name]), name
    assert got == fm.rankingScore(U, V, H, K, seen=S) or not eligible  # the same bits from run to run, whatever the chunk


def test_refusals():
    case, fm, U, V, scores = world(TU + 1, 2 * TV + 3)
    nU, nV = scores.shape
    L, h = capi.lib(), fm._push(U.ctx)
    ok, out = seen_dataset([[]] * nU, nV), np.zeros(5)
    ids, sc = np.zeros(nU, dtype=np.int64), np.zeros(nU)
    data, indices, indptr = csr_arrays([[(0, 1.0)]] * nU)
    F = nf.newCSRFieldDataset(data, indices, indptr, np.zeros(nU, dtype=np.int64), nU, nV, 1)
    twice = dataset([[(1, 1.0)], [(2, 1.0), (0, 1.0), (2, 1.0)]] + [[]] * (nU - 2), nV)
    bad = ((seen_dataset([[]] * nU, nV + 1), capi.ERR_INVALID, "seen must be nU x nV"), (seen_dataset([[]] * (nU - 1), nV), capi.ERR_INVALID, "seen must be nU x nV"),
           (nf.newCSRDataset(*csr_arrays([[]] * nU), nU, nV, ctx=nf.Context(0)), capi.ERR_INVALID, "seen must be nU x nV"), (F, capi.ERR_UNSUPPORTED, "field-aware"))
    for S, code, words in bad:
        for call in (lambda: L.nfm_cross_topk_seen(h, U.h, V.h, S.h, 1, 0, ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)),
                     lambda: L.nfm_cross_rank_metrics(h, U.h, V.h, S.h, ok.h, 1, 0, out.ctypes.data_as(C.c_void_p))):
            assert call() == code and words in L.nfm_last_error().decode()
        with pytest.raises((capi.NfmError, ValueError), match=words):
            fm.recommendUnseen(U, V, 1, seen=S)
    assert L.nfm_cross_topk_seen(h, U.h, V.h, None, 1, 0, None, None) == capi.ERR_INVALID
    assert L.nfm_cross_rank_metrics(h, U.h, V.h, None, twice.h, 1, 0, out.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID
    assert "row 1" in L.nfm_last_error().decode()
    with pytest.raises((capi.NfmError, ValueError), match="row 1"):
        fm.rankingScore(U, V, twice, 1)
    stream = nf.StreamCSRDataset.__new__(nf.StreamCSRDataset)
    stream.h = None
    for call in (lambda: fm.recommendUnseen(U, V, 1, seen=stream), lambda: fm.rankingScore(U, V, stream, 1), lambda: fm.rankingScore(U, V, ok, 1, seen=stream)):
        with pytest.raises(capi.NfmError, match="StreamCSRDataset") as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED
