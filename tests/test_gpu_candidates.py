"""-m gpu: sampleCandidates (nimfm_amd/csrc/candidates.hip) against the definition of include/nimfm_hip.h
restated in plain Python integers: every row of the result equals the restatement's, id for id."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import nimfm_amd as nf
from cross_cases import csr_arrays
from nimfm_amd import _capi as capi
from test_gpu_cross import dataset
from test_gpu_cross_pairs import world

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
CAND_MAX = int(re.search(r"kCandMax = (\d+);", open(os.path.join(os.path.dirname(capi.__file__), "csrc", "candidates.h")).read()).group(1))
SEEDS = (7, 0xF123456789ABCDEF)


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def restate_row(i, exc, inc, nV, nPer, seed):
    """row i of sampleCandidates, the definition word for word"""
    X = sorted(set(exc) | set(inc))
    E = nV - len(X)
    n = min(nPer, E)

    def elig(r):
        return r + next((p for p in range(len(X)) if X[p] - p > r), len(X))

    def first(m):
        got, t = [], 0
        while len(got) < m:
            v = (mix((seed + 0x9E3779B97F4A7C15 * ((i << 32) + t + 1)) & M64) * E) >> 64
            if v not in got:
                got.append(v)
            t += 1
        return got

    if n == E:
        S = [elig(r) for r in range(E)]
    elif 2 * n <= E:
        S = [elig(r) for r in first(n)]
    else:
        left_out = first(E - n)
        S = [elig(r) for r in range(E) if r not in left_out]
    assert len(set(S)) == n and not set(S) & set(X)
    return sorted(set(S) | set(inc))


def matrix(rows, nV):
    return dataset([[(j, 1.0) for j in r] for r in rows], nV)


@functools.lru_cache(maxsize=None)
def rows_of(nU, nV, n):
    """(exclude, include): an empty row; all but 3 items excluded; E just above 2 n (direct); n < E < 2 n (complement); an unsorted
    row with one id 70 times, ids 0 and nV - 1, a run of 64 and an include row that overlaps it.  One user: the last of them."""
    rng = np.random.RandomState(nV + n)
    pick = lambda m: [int(j) for j in rng.permutation(nV)[:max(0, min(m, nV))]]  # noqa: E731
    run = list(range(nV // 3, min(nV // 3 + 64, nV)))
    exc = [[], pick(nV - 3), pick(nV - 2 * n - 1), pick(nV - n - max(1, n // 2)), [run[0]] * 70 + [nV - 1] + run[::-1] + [0]]
    inc = [[], [], [j for j in range(nV) if j not in exc[2]][:5][::-1], [j for j in range(nV) if j not in exc[3]][1:3], run[:3] + pick(4) + run[:1]]
    return (exc, inc) if nU == 5 else (exc[-1:], inc[-1:])


def ids_of(Cm):
    indptr, indices, data, _ = Cm.to_host()
    assert np.all(data == 1.0) and Cm.rows_ascend()
    return [[int(j) for j in indices[a:b]] for a, b in zip(indptr[:-1], indptr[1:])]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", (1, 7, 64, 65, CAND_MAX))
@pytest.mark.parametrize("nV", (1, 63, 64, 65, 300))
@pytest.mark.parametrize("nU", (1, 5))
def test_rows_are_the_definition(nU, nV, n, seed):
    exc, inc = rows_of(nU, nV, n)
    Ex, In = matrix(exc, nV), matrix(inc, nV)
    for include, inc_rows in ((None, [[]] * nU), (In, inc)):
        want = [restate_row(i, exc[i], inc_rows[i], nV, n, seed) for i in range(nU)]
        Cm = nf.sampleCandidates(Ex, n, seed, include=include)
        got = ids_of(Cm)
        assert got == want
        for i, row in enumerate(got):  # the properties, directly
            assert all(a < b for a, b in zip(row, row[1:])) and set(inc_rows[i]) <= set(row) and not (set(row) & set(exc[i])) - set(inc_rows[i])
            assert len(row) == min(n, nV - len(set(exc[i]) | set(inc_rows[i]))) + len(set(inc_rows[i]))
    assert ids_of(nf.sampleCandidates(nf.toCSCDataset(Ex), n, seed, include=nf.toCSCDataset(In))) == got  # through the row twins
    again = nf.sampleCandidates(Ex, n, seed, include=In)  # a repeated call, by bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(Cm.to_host()[:3], again.to_host()[:3]))


@pytest.mark.parametrize("n_excluded,case", ((0, "direct"), (100, "complement")))
def test_a_full_list(n_excluded, case):
    """kCandMax draws fill every slot of the list: nV = 2100 gives E >= 2 kCandMax (direct) and, with 100 excluded, 976 left out"""
    exc = [[], list(range(5, 5 + n_excluded))]
    inc = [[3], [7, 2050]]
    got = ids_of(nf.sampleCandidates(matrix(exc, 2100), CAND_MAX, 11, include=matrix(inc, 2100)))
    assert got == [restate_row(i, exc[i], inc[i], 2100, CAND_MAX, 11) for i in range(2)]


def test_seeds_differ_and_ranking_score_among_reads_the_result():
    exc, inc = rows_of(5, 300, 7)
    Ex, In = matrix(exc, 300), matrix(inc, 300)
    one, two = (nf.sampleCandidates(Ex, 7, s, include=In) for s in SEEDS)
    assert ids_of(one) != ids_of(two)
    _, fm, U, V, _ = world(5, 300)
    mine = matrix([restate_row(i, exc[i], inc[i], 300, 7, SEEDS[0]) for i in range(5)], 300)
    held = matrix([sorted(set(r)) for r in inc], 300)
    got = fm.rankingScoreAmong(U, V, held, 5, one)
    assert got == fm.rankingScoreAmong(U, V, held, 5, mine) and got["nUsers"] == 3 and len(got) == 5


def test_refusals():
    L, h = capi.lib(), C.c_void_p()
    ok, wide = matrix([[0]] * 3, 70), matrix([[0]] * 3, 71)
    F = nf.newCSRFieldDataset(*csr_arrays([[(0, 1.0)]] * 3), np.zeros(3, dtype=np.int64), 3, 70, 1)
    other = nf.newCSRDataset(*csr_arrays([[(0, 1.0)]] * 3), 3, 70, ctx=nf.Context(0))
    for exclude, include, n, out, code, word in ((None, None, 1, h, capi.ERR_INVALID, "null exclude"), (ok, None, 1, None, capi.ERR_INVALID, "null out"),
                                                 (F, None, 1, h, capi.ERR_UNSUPPORTED, "exclude is a field-aware"),
                                                 (ok, F, 1, h, capi.ERR_UNSUPPORTED, "include is a field-aware"),
                                                 (ok, other, 1, h, capi.ERR_INVALID, "include belongs to another context"),
                                                 (ok, wide, 1, h, capi.ERR_INVALID, "include is 3 x 71 and exclude 3 x 70"),
                                                 (ok, None, 0, h, capi.ERR_INVALID, "nPerUser = 0"),
                                                 (ok, None, CAND_MAX + 1, h, capi.ERR_INVALID, "nPerUser = %d" % (CAND_MAX + 1))):
        rc = L.nfm_sample_candidates(exclude and exclude.h, include and include.h, n, 1, None if out is None else C.byref(out))
        assert rc == code and word in L.nfm_last_error().decode(), word
