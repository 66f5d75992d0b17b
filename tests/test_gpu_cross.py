"""-m gpu: crossDecisionFunction and recommend (nimfm_amd/csrc/cross.hip).

  1. crossDecisionFunction(U, V) against fm.decisionFunction(hstack(U[rep], V[tile])), the pairs made with the device ops, at
     the project's bound for decisionFunction against an independently ordered sum (tests/test_gpu_psgd_lazy.py:245);
  2. the bits of a score depend on its two rows alone: permutations and slices, by bytes;
  3. recommend is the top K, by (-score, id), of exactly those bits, whatever chunkItems is;
  4. recommend's ids are the restatement's (tests/cross_restatement.py) on every case of tests/cross_cases.py;
  5. every refusal, through the C ABI and the host, with its message;
  6. a call repeated gives the same bytes.
The tile's sizes come from nimfm_amd/csrc/cross.h (cross_cases.tile_shape()); no number of it is typed here."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cross_restatement as R
import nimfm_amd as nf
from cross_cases import cases, csr_arrays, make_case, make_rows, tile_shape
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
T = tile_shape()
TU, TV, KS = T["TU"], T["TV"], T["KS"]
CASES = cases()


def dataset(rows, d):
    data, indices, indptr = csr_arrays(rows)
    return nf.newCSRDataset(data, indices, indptr, len(rows), d)


def model(case):
    fm = nf.FactorizationMachine("regression", degree=2, nComponents=case["k"], fitLower=case["fitLower"], fitLinear=case["fitLinear"],
                                 fitIntercept=case["fitIntercept"])
    fm.set_params(np.asarray(case["P"])[None], case["w"], case["b"])
    fm.lams = np.asarray(case["lams"], dtype=np.float64)
    return fm


def up(case):
    return model(case), dataset(case["U"], case["dU"]), dataset(case["V"], case["dV"])


def pairs(fm, U, V):
    """the parent's only route: one row per pair, then decisionFunction"""
    nU, nV = U.nSamples, V.nSamples
    rep, til = np.repeat(np.arange(nU), nV), np.tile(np.arange(nV), nU)
    return fm.decisionFunction(nf.hstack(U[rep], V[til])).reshape(nU, nV)


def assert_close(got, want, what):
    err = np.abs(got - want) / (ATOL + RTOL * np.abs(want))
    print("%s: worst |cross - pairs| / bound = %.3g" % (what, err.max() if err.size else 0.0))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= ATOL + RTOL * np.abs(want)), what


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host_top(scores, K):
    """crossDecisionFunction's rows sorted on the host by (-score, id), NaN last"""
    ids = np.empty((scores.shape[0], K), dtype=np.int64)
    for i, row in enumerate(scores):
        nan = np.isnan(row)
        ids[i] = np.lexsort((np.arange(len(row)), np.where(nan, 0.0, -row), nan))[:K]
    return ids, np.take_along_axis(scores, ids, axis=1)


# ---- 1. against the pairs ----
@pytest.mark.parametrize("fitLower,fitLinear,fitIntercept", list(itertools.product(("explicit", "none", "augment"), (True, False), (True, False))))
def test_options_against_pairs(fitLower, fitLinear, fitIntercept):
    case = make_case("opt", 21, nU=TU + 1, nV=TV + 1, dU=9, dV=7, k=5, K=1, fitLower=fitLower, fitLinear=fitLinear, fitIntercept=fitIntercept, lams=True)
    fm, U, V = up(case)
    assert_close(fm.crossDecisionFunction(U, V), pairs(fm, U, V), "%s %s %s" % (fitLower, fitLinear, fitIntercept))


@pytest.mark.parametrize("k", sorted({1, 3, 64, 65, 128, 129, 200, KS - 1, KS, KS + 1}))
def test_n_components_against_pairs(k):
    case = make_case("k", 22 + k, nU=5, nV=TV + 1, dU=8, dV=6, k=k, K=1, fitLower="augment", fitLinear=False)
    fm, U, V = up(case)
    assert_close(fm.crossDecisionFunction(U, V), pairs(fm, U, V), "k = %d" % k)


@pytest.mark.parametrize("nU,nV", list(itertools.product((1, TU - 1, TU, TU + 1), (1, TV - 1, TV + 1, 2 * TV + 3))))
def test_tile_edges_against_pairs(nU, nV):
    case = make_case("edge", 1000 * nU + nV, nU=nU, nV=nV, dU=10, dV=12, k=6, K=1)
    fm, U, V = up(case)
    got = fm.crossDecisionFunction(U, V)
    assert_close(got, pairs(fm, U, V), "%d x %d" % (nU, nV))
    assert_close(got, np.array(R.cross(case)), "%d x %d against the restatement" % (nU, nV))


def test_tile_layout_on_exact_integers():
    """the matrix instruction's operand and result maps on data whose every sum is exact: small integers, V unlike U, so that a
    result in the wrong row or column is another number; equal to the restatement to the bit"""
    case = make_case("int", 33, nU=TU + 1, nV=TV + 3, dU=7, dV=9, k=5, K=1)
    rng = np.random.RandomState(7)
    for rows in (case["U"], case["V"]):
        for i, r in enumerate(rows):
            rows[i] = [(j, float(rng.randint(1, 4) * rng.choice([-1, 1]))) for j, _ in r]
    case["P"] = rng.randint(-3, 4, size=case["P"].shape).astype(np.float64)
    case["w"] = rng.randint(-5, 6, size=case["w"].shape).astype(np.float64)
    case["b"] = 3.0
    fm, U, V = up(case)
    want = np.array(R.cross(case))
    assert np.array_equal(want, np.rint(want)) and len(np.unique(want)) > 50
    assert np.array_equal(fm.crossDecisionFunction(U, V), want)
    assert np.array_equal(pairs(fm, U, V), want)


def test_row_shapes_are_in_the_cases():
    """an empty row, a one-entry row, unsorted ids and a repeated id on each side (tests/cross_cases.py: make_rows)"""
    case = make_case("rows", 31, nU=4, nV=5, dU=6, dV=6, k=4, K=1)
    for rows in (case["U"], case["V"]):
        assert rows[0] == [] and len(rows[1]) == 1
        ids = [j for j, _ in rows[2]]
        assert ids != sorted(ids) and len(set(ids)) < len(ids)
    fm, U, V = up(case)
    assert_close(fm.crossDecisionFunction(U, V), pairs(fm, U, V), "rows")


@pytest.mark.parametrize("csc_side", ("U", "V", "both"))
def test_column_major_datasets(csc_side):
    case = make_case("csc", 41, nU=TU + 3, nV=TV + 2, dU=9, dV=9, k=7, K=1, fitLower="augment", fitLinear=False)
    fm, U, V = up(case)
    Uc = nf.toCSCDataset(U) if csc_side in ("U", "both") else U
    Vc = nf.toCSCDataset(V) if csc_side in ("V", "both") else V
    # a CSCDataset is read through its row twin, as decisionFunction reads it: the rows of toCSRDataset
    Ur = nf.toCSRDataset(Uc) if Uc is not U else U
    Vr = nf.toCSRDataset(Vc) if Vc is not V else V
    got = fm.crossDecisionFunction(Uc, Vc)
    assert_close(got, pairs(fm, Ur, Vr), "csc " + csc_side)
    assert same_bytes(got, fm.crossDecisionFunction(Ur, Vr))


# ---- 2. position independence ----
def test_scores_do_not_depend_on_position():
    case = make_case("pos", 51, nU=2 * TU + 5, nV=2 * TV + 9, dU=11, dV=13, k=KS + 3, K=1, lams=True)
    fm, U, V = up(case)
    full = fm.crossDecisionFunction(U, V)
    rng = np.random.RandomState(5)
    for _ in range(2):
        p, q = rng.permutation(U.nSamples), rng.permutation(V.nSamples)
        assert same_bytes(fm.crossDecisionFunction(U[p], V[q]), np.ascontiguousarray(full[p][:, q]))
    for a, b in ((TU - 3, TV + 5), (1, 1), (TU + 1, 7)):
        assert same_bytes(fm.crossDecisionFunction(U[0:a], V[0:b]), np.ascontiguousarray(full[:a, :b]))
    assert same_bytes(fm.crossDecisionFunction(U, V), full)  # 6. the same call again


def long_rows(rng, n, d, lo, hi):
    """n rows of lo .. hi entries each, ids unsorted and repeated: long enough for the order of a row's sum to show"""
    return [[(int(j), float(x)) for j, x in zip(rng.randint(0, d, size=m), rng.uniform(-1.5, 1.5, size=m))]
            for m in rng.randint(lo, hi + 1, size=n)]


@pytest.mark.parametrize("big_side", ("U", "V"))
def test_scores_do_not_depend_on_the_size_of_the_set(big_side):
    """A row's sums are ordered by the model's lanes per row alone.  decisionFunction's own launch picks its row slots from the
    number of rows and their mean length (lane_map.h: choose_split; k = 6: 16 slots up to 4096 rows, 8 at 8192); the sides of
    the cross must not: half of a set of 8192 rows, and a handful of them, scored alone, give the bytes of the whole."""
    rng = np.random.RandomState(17)
    n, few, d, k = 8192, 3, 24, 6
    big, small = long_rows(rng, n, d, 9, 40), long_rows(rng, few, d, 9, 40)
    case = make_case("size", 52, nU=1, nV=1, dU=d, dV=d, k=k, K=1)
    case["U"], case["V"] = (big, small) if big_side == "U" else (small, big)
    fm, U, V = up(case)
    full = fm.crossDecisionFunction(U, V)
    for a, b in ((0, n // 2), (n // 2, n), (n - 5, n), (100, 101)):
        part = fm.crossDecisionFunction(U[a:b], V) if big_side == "U" else fm.crossDecisionFunction(U, V[a:b])
        want = full[a:b] if big_side == "U" else full[:, a:b]
        assert same_bytes(part, np.ascontiguousarray(want)), (a, b)
    rows = (big[100:101], small) if big_side == "U" else (small, big[100:101])
    assert_close(full[100:101] if big_side == "U" else full[:, 100:101], np.array(R.cross(dict(case, U=rows[0], V=rows[1]))), "one row of the large set")


@pytest.mark.parametrize("long_side", ("U", "V"))
def test_scores_do_not_depend_on_a_long_neighbour(long_side):
    """one row of 6000 entries among 40 short ones moves the set's mean row length past choose_split's latency rule (mean / 32);
    the short rows score what they score without it, and the long row what it scores alone"""
    rng = np.random.RandomState(18)
    d, k = 30, 6
    short, other = long_rows(rng, 40, d, 9, 20), long_rows(rng, 4, d, 9, 20)
    long_row = long_rows(rng, 1, d, 6000, 6000)
    mixed = short[:20] + long_row + short[20:]
    case = make_case("long", 53, nU=1, nV=1, dU=d, dV=d, k=k, K=1)

    def score(rows):
        c = dict(case, U=rows, V=other) if long_side == "U" else dict(case, U=other, V=rows)
        fm, U, V = up(c)
        out = fm.crossDecisionFunction(U, V)
        return out if long_side == "U" else np.ascontiguousarray(out.T)

    with_long, without, alone = score(mixed), score(short), score(long_row)
    assert same_bytes(np.ascontiguousarray(np.delete(with_long, 20, axis=0)), without)
    assert same_bytes(np.ascontiguousarray(with_long[20:21]), alone)


def test_host_copy_in_several_blocks():
    """3000 x 3000 scores are more than one 64 MiB block of users: the blocks leave one after the other through the pinned pair
    (nfm_cross_decision_function), and are the bytes of the same users scored in calls of one block each"""
    rng = np.random.RandomState(19)
    n, d = 3000, 40
    case = make_case("blocks", 54, nU=1, nV=1, dU=d, dV=d, k=5, K=1)
    case["U"], case["V"] = long_rows(rng, n, d, 1, 6), long_rows(rng, n, d, 1, 6)
    fm, U, V = up(case)
    assert n * n * 8 > 64 << 20 and (n // 2) * n * 8 < 64 << 20
    full = fm.crossDecisionFunction(U, V)
    halves = np.concatenate([fm.crossDecisionFunction(U[0:n // 2], V), fm.crossDecisionFunction(U[n // 2:n], V)])
    assert same_bytes(full, halves)
    ids, sc = fm.recommend(U[0:TU], V, 3)
    want_ids, want_scores = host_top(full[:TU], 3)
    assert np.array_equal(ids, want_ids) and same_bytes(sc, want_scores)


# ---- 3. recommend against crossDecisionFunction ----
@pytest.fixture(scope="module")
def ranked():
    case = make_case("rank", 61, nU=TU + 2, nV=2 * TV + 3, dU=8, dV=10, k=9, K=7, tie=40)
    fm, U, V = up(case)
    return case, fm, U, V, fm.crossDecisionFunction(U, V)


@pytest.mark.parametrize("K", (1, 2, 7, "nV"))
def test_recommend_is_the_sorted_scores(ranked, K):
    case, fm, U, V, scores = ranked
    nV = V.nSamples
    K = nV if K == "nV" else K
    want_ids, want_scores = host_top(scores, K)
    first = None
    for chunk in (0, 1, TV, nV - 1):
        ids, sc = fm.recommend(U, V, K, chunkItems=chunk)
        assert ids.dtype == np.int64 and np.array_equal(ids, want_ids), chunk
        assert same_bytes(sc, want_scores), chunk
        first = first or (ids, sc)
    assert same_bytes(fm.recommend(U, V, K)[1], first[1]) and same_bytes(fm.recommend(U, V, K)[0], first[0])


def test_recommend_resolves_the_planted_tie_by_id(ranked):
    case, fm, U, V, scores = ranked
    a, b = case["tie"]
    assert a < b and same_bytes(scores[:, a], scores[:, b])
    for chunk in (0, TV):  # one chunk, and the two items in different chunks or tiles
        ids, _ = fm.recommend(U, V, 7, chunkItems=chunk)
        row = list(ids[-1])  # the last user's best item is the planted one
        assert row[0] == a and row[1] == b
        for r in ids:
            if a in r and b in r:
                assert list(r).index(a) + 1 == list(r).index(b)


def test_recommend_256_of_300():
    case = make_case("k256", 71, nU=3, nV=300, dU=6, dV=14, k=4, K=256)
    fm, U, V = up(case)
    scores = fm.crossDecisionFunction(U, V)
    want_ids, want_scores = host_top(scores, 256)
    for chunk in (0, TV):
        ids, sc = fm.recommend(U, V, 256, chunkItems=chunk)
        assert np.array_equal(ids, want_ids) and same_bytes(sc, want_scores)


def test_nan_scores_rank_last():
    case = make_case("nan", 81, nU=TU + 1, nV=TV + 7, dU=5, dV=6, k=3, K=1)
    case["P"][1, case["dU"] + 2] = np.nan  # items that hold feature 2 of V score NaN
    fm, U, V = up(case)
    scores = fm.crossDecisionFunction(U, V)
    nan_items = [j for j, row in enumerate(case["V"]) if any(c == 2 for c, _ in row)]
    assert 0 < len(nan_items) < V.nSamples
    assert np.array_equal(np.isnan(scores), np.isin(np.arange(V.nSamples), nan_items)[None].repeat(U.nSamples, 0))
    nV = V.nSamples
    want_ids, want_scores = host_top(scores, nV)
    for chunk in (0, TV):
        ids, sc = fm.recommend(U, V, nV, chunkItems=chunk)
        assert np.array_equal(ids, want_ids) and same_bytes(sc, want_scores)
        assert np.array_equal(ids[:, nV - len(nan_items):], np.array(nan_items)[None].repeat(U.nSamples, 0))


# ---- 4. against the restatement ----
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_recommend_ids_are_the_restatement_s(case):
    fm, U, V = up(case)
    assert_close(fm.crossDecisionFunction(U, V), np.array(R.cross(case)), case["name"])
    want = np.array([[j for j, _ in R.rank(row, case["K"])] for row in R.cross(case)], dtype=np.int64)
    for chunk in (0, 1):
        ids, _ = fm.recommend(U, V, case["K"], chunkItems=chunk)
        assert np.array_equal(ids, want), (case["name"], chunk)


# ---- 5. refusals ----
def refused(fm_handle, U, V, code, *words):
    """the three entry points through the C ABI: the code and the message"""
    L = capi.lib()
    out = np.zeros(max(1, U.nSamples * V.nSamples))
    ids = np.zeros(max(1, U.nSamples), dtype=np.int64)
    for call in (lambda: L.nfm_cross_decision_function(fm_handle, U.h, V.h, out.ctypes.data_as(C.c_void_p)),
                 lambda: L.nfm_cross_decision_function_device(fm_handle, U.h, V.h, None),
                 lambda: L.nfm_cross_topk(fm_handle, U.h, V.h, 1, 0, ids.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))):
        assert call() == code
        msg = L.nfm_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)


def small_sets(dU=4, dV=5):
    rng = np.random.RandomState(3)
    return dataset(make_rows(rng, 3, dU, 2), dU), dataset(make_rows(rng, 4, dV, 2), dV)


def test_refusals_of_models():
    U, V = small_sets()
    d = U.nFeatures + V.nFeatures
    way = ("hstack(U[rep], V[tile])", "decisionFunction")
    fm3 = nf.FactorizationMachine("r", degree=3, nComponents=2)
    fm3.set_params(np.ones((2, 2, d)), np.zeros(d), 0.0)
    refused(fm3._push(U.ctx), U, V, capi.ERR_UNSUPPORTED, "degree 2", *way)
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=2)
    ffm.set_params(np.ones((2, d, 2)), np.zeros(d), 0.0)
    refused(ffm._push(U.ctx), U, V, capi.ERR_UNSUPPORTED, "field-aware model", *way)
    cfm = nf.ConvexFactorizationMachine("r", maxComponents=2)
    cfm.set_params(np.ones((1, d)), np.ones(1), np.zeros(d), 0.0)
    refused(cfm._push(U.ctx), U, V, capi.ERR_UNSUPPORTED, "ConvexFactorizationMachine", *way)
    # the host: the two calls are FactorizationMachine's; the other kinds have none, their handles are refused above
    with pytest.raises(capi.NfmError, match="degree 2") as e:
        fm3.crossDecisionFunction(U, V)
    assert e.value.code == capi.ERR_UNSUPPORTED and "decisionFunction" in str(e.value)
    with pytest.raises(capi.NfmError, match="degree 2"):
        fm3.recommend(U, V, 1)
    for m in (ffm, cfm):
        assert not hasattr(m, "crossDecisionFunction") and not hasattr(m, "recommend")


def test_refusals_of_datasets():
    U, V = small_sets()
    d = U.nFeatures + V.nFeatures
    fm = nf.FactorizationMachine("r", nComponents=2)
    fm.set_params(np.ones((1, 2, d)), np.zeros(d), 0.0)
    h = fm._push(U.ctx)
    way = ("hstack(U[rep], V[tile])", "decisionFunction")
    F = nf.newCSRFieldDataset(np.ones(2), np.array([0, 1]), np.array([0, 1, 2]), np.array([0, 1]), 2, U.nFeatures, 2)
    refused(h, F, V, capi.ERR_UNSUPPORTED, "field-aware dataset", *way)
    refused(h, U, F, capi.ERR_UNSUPPORTED, "field-aware dataset", *way)
    with pytest.raises(capi.NfmError, match="field-aware dataset"):
        fm.crossDecisionFunction(F, V)
    # a dataset used in row blocks has no resident handle: the host refuses it
    S = nf.StreamCSRDataset.__new__(nf.StreamCSRDataset)
    S.h = None
    for call in (lambda: fm.crossDecisionFunction(S, V), lambda: fm.crossDecisionFunction(U, S), lambda: fm.recommend(U, S, 1)):
        with pytest.raises(capi.NfmError, match="StreamCSRDataset") as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and "decisionFunction" in str(e.value)
    # U and V of different contexts
    other = nf.Context(0)
    data, indices, indptr = csr_arrays([[(0, 1.0)], []])
    V2 = nf.newCSRDataset(data, indices, indptr, 2, V.nFeatures, ctx=other)
    refused(h, U, V2, capi.ERR_UNSUPPORTED, "different contexts", *way)
    with pytest.raises(capi.NfmError, match="different contexts"):
        fm.recommend(U, V2, 1)
    # the widths
    W = dataset([[(0, 1.0)]], V.nFeatures + 1)
    refused(h, U, W, capi.ERR_INVALID, "Invalid nFeatures.")
    with pytest.raises(ValueError, match="Invalid nFeatures."):
        fm.crossDecisionFunction(U, W)
    with pytest.raises(capi.NotFittedError):
        nf.FactorizationMachine("r").crossDecisionFunction(U, V)


def test_top_k_bounds():
    case = make_case("bounds", 91, nU=2, nV=300, dU=3, dV=4, k=2, K=1)
    fm, U, V = up(case)
    small = dataset(case["V"][:5], case["dV"])
    for ds, K in ((V, 0), (V, -1), (V, 257), (small, 6)):
        with pytest.raises(ValueError, match="crossDecisionFunction") as e:
            fm.recommend(U, ds, K)
        assert "min(nV, 256) = %d" % min(ds.nSamples, 256) in str(e.value)
    assert fm.recommend(U, small, 5)[0].shape == (2, 5) and fm.recommend(U, V, 256)[0].shape == (2, 256)
