"""-m gpu: the Ranker (nimfm_amd/csrc/cross.hip: k_cross_side_ffm, api.hip: nfm_ranker_*).  Field-aware
scores against the reference's double loop on the joined row (model/field_aware_factorization_machine.nim:52-76), restated below
in float64 numpy, at rtol 1e-9 / atol 1e-12 (decisionFunction against an independently ordered sum);
everything else by bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import nimfm_amd as nf
from cross_cases import make_case
from nimfm_amd import _capi as capi
from test_gpu_cross import dataset, host_top, same_bytes, up
from test_gpu_rank_of import matrix, want

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12


def joined_score(P, w, b, row):
    """b + sum w_j x_j + sum_{j1 < j2} x1 x2 <P[f2, j1], P[f1, j2]> over the entries (j, f, x) of one row"""
    j, f, x = (np.array(c) for c in zip(*row)) if row else (np.zeros(0, dtype=int),) * 2 + (np.zeros(0),)
    G = P[f[None, :], j[:, None]]  # G[a, c] = P[f_c, j_a]
    pair = (x[:, None] * x[None, :]) * np.einsum("ack,cak->ac", G, G)
    return b + float(np.sum(w[j] * x)) + float(np.sum(pair[j[:, None] < j[None, :]]))


def restatement(P, w, b, U, V, dU, FU):
    return np.array([[joined_score(P, w, b, u + [(dU + j, FU + f, x) for j, f, x in v]) for v in V] for u in U])


def field_rows(rng, n, d, F, long_row):
    """rows of (column, field, value) in random (unsorted) storage order, several entries per field"""
    rows = []
    for i in range(n):
        m = 150 if i == 5 and long_row else int(rng.randint(1, 2 * F + 3))
        rows.append([(int(rng.randint(d)), int(rng.randint(F)), float(rng.uniform(-1, 1))) for _ in range(m)])
    rows[0] = []  # an empty row
    rows[1] = [(int(rng.randint(d)), f, 0.5 + f) for f in range(F) for _ in range(2)]  # every field, twice
    rows[2] = [(j, F - 1, x) for j, f, x in rows[2]]  # right after it: no entry of any field but the last
    rows[3] = rows[3] + [(rows[3][0][0], int(rng.randint(F)), -0.75)]  # a column id repeated inside the row
    return rows


def field_dataset(rows, d, F):
    indptr = np.cumsum([0] + [len(r) for r in rows])
    col = lambda c, t: np.array([e[c] for r in rows for e in r], dtype=t)  # noqa: E731
    return nf.newCSRFieldDataset(col(2, np.float64), col(0, np.int64), indptr, col(1, np.int64), len(rows), d, F)


@functools.lru_cache(maxsize=None)
def ffm_world(FU, FV, k, nU=33, nV=65, dU=11, dV=7):
    rng = np.random.RandomState(100 * FU + 10 * FV + k)
    P, w, b = rng.normal(size=(FU + FV, dU + dV, k)) * 0.3, rng.normal(size=dU + dV), 0.37
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=k)
    ffm.set_params(P, w, b)
    Ur, Vr = field_rows(rng, nU, dU, FU, k <= 8), field_rows(rng, nV, dV, FV, False)
    U, V = field_dataset(Ur, dU, FU), field_dataset(Vr, dV, FV)
    return ffm, U, V, Ur, Vr, nf.newRanker(ffm, U, V)


SPLITS = ((1, 1, 1), (2, 3, 4), (3, 2, 5), (4, 4, 8), (1, 5, 33), (8, 8, 64))  # odd k: padding; 33: the next lane width; the cap, 4096


@pytest.mark.parametrize("FU,FV,k", SPLITS)
def test_field_aware_scores(FU, FV, k):
    ffm, U, V, Ur, Vr, R = ffm_world(FU, FV, k)
    got, ref = R.scores(), restatement(ffm.P, ffm.w, ffm.intercept, Ur, Vr, U.nFeatures, FU)
    rep, til = np.repeat(np.arange(33), 65), np.tile(np.arange(65), 33)
    pairs = ffm.decisionFunction(nf.hstack(U[rep], V[til])).reshape(33, 65)
    for name, other in (("restatement", ref), ("decisionFunction of the pairs", pairs)):
        err = np.abs(got - other) / (ATOL + RTOL * np.abs(other))
        print("%s: worst |scores - it| / bound = %.3g" % (name, err.max()))
        assert got.shape == other.shape == (33, 65) and err.max() <= 1.0, name
    assert (R.nUsers, R.nItems) == (33, 65)


@pytest.mark.parametrize("FU,FV,k", ((2, 3, 4), (1, 5, 33), (8, 8, 64)))
def test_side_bits_depend_on_the_row_alone(FU, FV, k):
    ffm, U, V, _, _, R = ffm_world(FU, FV, k)
    rng = np.random.RandomState(k)
    pu, pv = rng.permutation(33)[:20], rng.permutation(65)[:40]
    assert same_bytes(nf.newRanker(ffm, U[pu], V[pv]).scores(), np.ascontiguousarray(R.scores()[pu][:, pv]))


def test_side_bits_beyond_one_grid_pass():
    """40 000 users of two entries: more rows than one pass of the side kernel's grid holds"""
    rng = np.random.RandomState(5)
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=3)
    ffm.set_params(rng.normal(size=(3, 9, 3)), rng.normal(size=9), -0.2)
    Ur = [[(int(rng.randint(6)), int(rng.randint(2)), float(rng.uniform(-1, 1))) for _ in range(2)] for _ in range(40000)]
    U, V = field_dataset(Ur, 6, 2), field_dataset([[(0, 0, 1.0)], [(2, 0, -0.5), (1, 0, 0.25)], []], 3, 1)
    full = nf.newRanker(ffm, U, V).scores()
    for i in (0, 1, 4095, 4096, 16383, 32767, 32768, 36001, 39999):
        assert same_bytes(nf.newRanker(ffm, U[np.array([i])], V).scores(), full[i:i + 1]), i


def held_and_seen(rng, nU, nV):
    held = [[int(j) for j in rng.randint(0, nV, size=rng.randint(0, 5))] for _ in range(nU)]
    seen = [[int(j) for j in rng.randint(0, nV, size=rng.randint(0, 9))] for _ in range(nU)]
    seen[1] = list(range(nV - 2))  # fewer candidates than K
    return held, seen


@pytest.mark.parametrize("k", (3, 64, 150))
@pytest.mark.parametrize("fitLower", ("explicit", "augment", "none"))
def test_degree_two_ranker_is_the_existing_path(fitLower, k):
    case = make_case("ranker", 900 + k, nU=33, nV=65, dU=8, dV=10, k=k, K=1, fitLower=fitLower, lams=True)
    fm, U, V = up(case)
    R = nf.newRanker(fm, U, V)
    held, seen = held_and_seen(np.random.RandomState(k), 33, 65)
    H, S = matrix(held, 65), matrix(seen, 65)
    assert same_bytes(R.scores(), fm.crossDecisionFunction(U, V))
    assert same_bytes(R.scoresAt(H), fm.crossDecisionFunctionAt(U, V, H))
    for got, ref in ((R.recommend(10, S), fm.recommendUnseen(U, V, 10, S)), (R.recommend(65), fm.recommend(U, V, 65)),
                     (R.rankOf(H, S), fm.rankOf(U, V, H, S)), (R.rankOf(H), fm.rankOf(U, V, H))):
        assert same_bytes(got[0], ref[0]) and same_bytes(got[1], ref[1])


@pytest.mark.parametrize("chunk", (0, 64))
@pytest.mark.parametrize("with_seen", (False, True))
def test_field_aware_lists_and_ranks_follow_from_the_scores(with_seen, chunk):
    _, _, _, _, _, R = ffm_world(3, 2, 5)
    scores, K = R.scores(), 12
    held, seen = held_and_seen(np.random.RandomState(3), 33, 65)
    if not with_seen:
        seen = [[]] * 33
    H, S = matrix(held, 65), matrix(seen, 65) if with_seen else None
    ids, sc = R.recommend(K, S, chunk)
    order, _ = host_top(scores, 65)  # every item by (-score, id)
    for i in range(33):
        keep = [j for j in order[i] if j not in seen[i]][:K]
        assert list(ids[i]) == keep + [-1] * (K - len(keep)), i
        assert sc[i, :len(keep)].tobytes() == scores[i, keep].tobytes() and np.isnan(sc[i, len(keep):]).all(), i
    ranks, cand = want(scores, held, seen)
    got = R.rankOf(H, S, chunk)
    assert same_bytes(got[0], ranks) and same_bytes(got[1], cand)
    rows = np.repeat(np.arange(33), [len(r) for r in held])
    assert same_bytes(R.scoresAt(H), scores[rows, [j for r in held for j in r]])


def refusal_cases():
    ffm, U, V, _, _, _ = ffm_world(2, 3, 4)
    plainU, plainV = dataset([[(0, 1.0)]] * 2, 11), dataset([[(1, 1.0)]] * 3, 7)
    fm = nf.FactorizationMachine("r", nComponents=2)
    fm.set_params(np.ones((1, 2, 18)), np.zeros(18), 0.0)
    fm3 = nf.FactorizationMachine("r", degree=3, nComponents=2)
    fm3.set_params(np.ones((2, 2, 18)), np.zeros(18), 0.0)
    cfm = nf.ConvexFactorizationMachine("r", maxComponents=2)
    cfm.set_params(np.ones((2, 18)), np.ones(2), np.zeros(18), 0.0)
    wide = nf.FieldAwareFactorizationMachine("r", nComponents=64)
    wide.set_params(np.ones((18, 4, 64)), np.zeros(4), 0.0)
    one = lambda F, d: field_dataset([[(0, F - 1, 1.0)]], d, F)  # noqa: E731
    raw = nf.FactorizationMachine("r", nComponents=2)
    raw._d = 18
    return ((fm3, plainU, plainV, capi.ERR_UNSUPPORTED, "degree 2"), (cfm, plainU, plainV, capi.ERR_UNSUPPORTED, "Convex"),
            (ffm, plainU, plainV, capi.ERR_UNSUPPORTED, "field-aware datasets"), (fm, U, V, capi.ERR_UNSUPPORTED, "field-aware dataset"),
            (ffm, U, one(2, 7), capi.ERR_INVALID, "Invalid nFields."), (ffm, U, one(3, 8), capi.ERR_INVALID, "Invalid nFeatures."),
            (wide, one(9, 2), one(9, 2), capi.ERR_UNSUPPORTED, "decisionFunction"), (raw, plainU, plainV, capi.ERR_NOT_FITTED, "not fitted"))


@pytest.mark.parametrize("n", range(8))
def test_refusals(n):
    m, U, V, code, word = refusal_cases()[n]
    h, out = m._handle(U.ctx) if not m.isInitialized else m._push(U.ctx), C.c_void_p()
    assert capi.lib().nfm_ranker_create(h, U.h, V.h, C.byref(out)) == code and word in capi.lib().nfm_last_error().decode(), word
    assert not out.value


@pytest.mark.parametrize("kind", ("ffm", "fm"))
def test_ranker_is_a_snapshot(kind):
    if kind == "ffm":
        m, U, V, _, _, _ = ffm_world(2, 3, 4)
    else:
        m, U, V = up(make_case("snap", 77, nU=5, nV=9, dU=8, dV=10, k=4, K=1))
    R, old = nf.newRanker(m, U, V), (m.P.copy(), m.w.copy(), m.intercept)
    before = R.scores()
    m.set_params(2.0 * old[0], old[1] + 1.0, 1.5)
    later = nf.newRanker(m, U, V).scores()
    m.set_params(*old)  # (ffm_world is shared)
    assert same_bytes(R.scores(), before) and not np.array_equal(later, before)
