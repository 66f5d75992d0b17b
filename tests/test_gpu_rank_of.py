"""-m gpu: rankOf (nimfm_amd/csrc/cross.hip: k_cross_rank_of) against exact integer counts over the matrix
that crossDecisionFunction returns, under rank_key / ranks_before restated on uint64.  Integers throughout: no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import nimfm_amd as nf
from cross_cases import csr_arrays, make_case, tile_shape
from nimfm_amd import _capi as capi
from test_gpu_cross import dataset, same_bytes, up

pytestmark = pytest.mark.gpu
T = tile_shape()
TU, TV, KS = T["TU"], T["TV"], T["KS"]
SIGN = np.uint64(1) << np.uint64(63)


def rank_key(scores):
    """cross.hip: the bits as an unsigned integer that ascends with the number; -0 == +0; NaN -> 0"""
    b = np.ascontiguousarray(scores).view(np.uint64)
    k = np.where(b >> np.uint64(63), ~b, b | SIGN)
    return np.where(np.isnan(scores), np.uint64(0), np.where(scores == 0.0, SIGN, k))


def want(scores, held, seen):
    """(ranks in the rows' order, nCandidates): the unseen items j' with key > key[j], or the same key and a smaller id"""
    ids, ranks, cand = np.arange(scores.shape[1]), [], []
    for i, row in enumerate(held):
        k, unseen = rank_key(scores[i]), ~np.isin(ids, seen[i])
        cand.append(int(unseen.sum()))
        ranks += [int((unseen & ((k > k[j]) | ((k == k[j]) & (ids < j)))).sum()) if unseen[j] else -1 for j in row]
    return np.array(ranks, dtype=np.int64), np.array(cand, dtype=np.int64)


def matrix(rows, nV):
    return dataset([[(j, float(n % 2)) for n, j in enumerate(r)] for r in rows], nV)  # the values, zeros too, mean nothing


@functools.lru_cache(maxsize=None)
def world(nU, nV, k):
    """model, sets, scores (a NaN parameter with the wider k), and the held-out and seen rows"""
    case = make_case("rank", 7000 + nU + nV + k, nU=nU, nV=nV, dU=8, dV=10, k=k, K=1, tie=40 if nV > 41 else None)
    if k > KS:
        case["P"][0, case["dU"] + 2] = np.nan  # items that hold feature 2 of V score NaN (test_gpu_cross.py)
    fm, U, V = up(case)
    rng = np.random.RandomState(nU + nV)
    edges = [j for j in (0, TV - 1, TV, 2 * TV - 1, 2 * TV, nV - 1) if j < nV]
    pick = lambda m: (edges + [int(j) for j in rng.randint(0, nV, size=m)])[:m]  # noqa: E731  (repeats where nV is small)
    at = {0: [], 1: pick(1), 2: sorted(pick(63)), 5: pick(7)[::-1], 9: pick(64), TU - 1: pick(65), TU: pick(130)}  # row 5: unsorted
    held = [at.get(i, []) for i in range(TU + 1)]
    if case["tie"]:
        held[-1] = held[-1] + list(case["tie"])[::-1]  # both of the planted tie, the larger id first
    every = list(range(nV))
    sat = {0: edges, 1: every[:TV], 2: held[2][:1] + edges, 9: [nV // 2] * 70 + [0], TU - 1: [j for j in every if j not in (held[TU - 1][0], nV - 1)],
           TU: every[TV:2 * TV] + held[TU][3:5]}
    seen = [sat.get(i, []) for i in range(TU + 1)]
    if nU == 1:  # one user: every held-out row in one, the sparse seen rows in one
        held, seen = [sum(held, [])], [seen[0] + seen[2] + seen[9]]
    return case, fm, U, V, fm.crossDecisionFunction(U, V), held, seen


@pytest.mark.parametrize("k", (KS - 1, KS + 1))
@pytest.mark.parametrize("nV", (1, TV - 1, TV + 1, 2 * TV + 3, 300))
@pytest.mark.parametrize("nU", (1, TU + 1))
def test_ranks_are_the_counts(nU, nV, k):
    case, fm, U, V, scores, held, seen = world(nU, nV, k)
    assert bool(np.isnan(scores).any()) == (k > KS) or nV == 1
    H, K = matrix(held, nV), min(nV, 256)
    for name, srows in (("none", None), ("empty", [[]] * nU), ("seen", seen)):
        S = None if srows is None else matrix(srows, nV)
        ranks, cand = want(scores, held, srows or [[]] * nU)
        for chunk in sorted({0, 1, TV, nV - 1}):
            got = fm.rankOf(U, V, H, seen=S, chunkItems=chunk)
            assert same_bytes(got[0], ranks) and same_bytes(got[1], cand), (name, chunk, got[0], ranks)
        assert all(same_bytes(a, b) for a, b in zip(fm.rankOf(U, V, H, seen=S), (ranks, cand))), name  # a repeated call
        assert (name == "seen") == bool((ranks == -1).any())
        # the rank is the item's place in the list
        ids, _ = fm.recommendUnseen(U, V, K, seen=S)
        rows = np.repeat(np.arange(nU), [len(r) for r in held])
        cols = np.array([j for r in held for j in r], dtype=np.int64)
        inside = (ranks >= 0) & (ranks < K)
        assert np.array_equal(ids[rows[inside], ranks[inside]], cols[inside]), name
        # column-major sets are read through their row twins: the entries in toCSRDataset's order
        Hc = nf.toCSCDataset(H)
        indptr, indices, _, _ = nf.toCSRDataset(Hc).to_host()
        twin = [[int(j) for j in indices[indptr[i]:indptr[i + 1]]] for i in range(nU)]
        got = fm.rankOf(U, V, Hc, seen=None if S is None else nf.toCSCDataset(S))
        assert same_bytes(got[0], want(scores, twin, srows or [[]] * nU)[0]) and same_bytes(got[1], cand), name
    if case["tie"]:  # equal bits: the smaller id first, between them only items of the same key (NaN against NaN goes by id)
        a, b = case["tie"]
        rb, ra = fm.rankOf(U, V, matrix([[]] * (nU - 1) + [[b, a]], nV))[0]
        key = rank_key(scores[-1])
        assert scores[-1, a].tobytes() == scores[-1, b].tobytes() and rb == ra + 1 + int((key[a + 1:b] == key[a]).sum())


def test_refusals():
    _, fm, U, V, _, _, _ = world(TU + 1, TV + 1, KS - 1)
    nU, nV = TU + 1, TV + 1
    L, h, vp = capi.lib(), fm._push(U.ctx), lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok, ranks, cand = matrix([[0]] * nU, nV), np.zeros(nU, dtype=np.int64), np.zeros(nU, dtype=np.int64)
    F = nf.newCSRFieldDataset(*csr_arrays([[(0, 1.0)]] * nU), np.zeros(nU, dtype=np.int64), nU, nV, 1)
    fm3 = nf.FactorizationMachine("r", degree=3, nComponents=2)
    fm3.set_params(np.ones((2, 2, 18)), np.zeros(18), 0.0)
    for m, X, code, word in ((h, matrix([[0]] * nU, nV + 1), capi.ERR_INVALID, "heldOut must be nU x nV"), (h, F, capi.ERR_UNSUPPORTED, "field-aware"),
                             (fm3._push(U.ctx), ok, capi.ERR_UNSUPPORTED, "degree 2")):
        assert L.nfm_cross_rank_of(m, U.h, V.h, X.h, None, 0, vp(ranks), vp(cand)) == code and word in L.nfm_last_error().decode(), word
