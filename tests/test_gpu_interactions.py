"""-m gpu: interactionStats and topInteractions (nimfm_amd/csrc/interactions.hip) against numpy in float64,
W = (Q * lams) @ Q.T with Q = P[order].T:
  1. integer parameters, where every product and sum is exact in any order: all five numbers and the whole ranking are numpy's;
  2. Gaussian parameters with a planted pattern: the counts and the ranked pairs are numpy's, the sums within rtol 1e-9;
  3. a call repeated gives the same bytes, and which zero rows are interleaved does not change the counts;
  4. every refusal, through the C ABI.
The tile's edge comes from nimfm_amd/csrc/interactions.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc", "interactions.h")).read()
T, GRID_PER_CU = (int(re.search(r"constexpr int %s = (\d+);" % n, _H).group(1)) for n in ("kInterT", "kInterGridPerCU"))
N_CU = 256  # an MI355X
RTOL = 1e-9  # the project's bound for an independently ordered sum
KS = (1, 7, 256)


def reference(fm, order, K):
    Q = fm.P[order].T
    W = (Q * fm.lams) @ Q.T
    n = len(W)
    off = (W != 0) & ~np.eye(n, dtype=bool)  # NaN != 0; -0 == 0
    i, j = np.triu_indices(n, 1)
    w = W[i, j]
    used = np.flatnonzero(off[i, j])
    key = np.where(np.isnan(w[used]), -1.0, np.abs(w[used]))
    best = used[np.lexsort((j[used], i[used], -key))][:K]
    pairs, weights = np.full((K, 2), -1, dtype=np.int64), np.full(K, np.nan)
    pairs[:len(best), 0], pairs[:len(best), 1], weights[:len(best)] = i[best], j[best], w[best]
    stats = {"l1Norm": np.abs(W).sum(), "l1OffDiag": np.abs(W * ~np.eye(n, dtype=bool)).sum(), "nInteractions": len(used),
             "nFeatures": int(off.any(1).sum()), "nNonzeroRows": int((Q != 0).any(1).sum())}
    return stats, pairs, weights


def model(P, fitLower="explicit", lams=None):
    fm = nf.FactorizationMachine("r", degree=3, nComponents=P.shape[1], fitLower=fitLower)
    fm.set_params(P, np.zeros(P.shape[2] - fm.nAugments), 0.0)
    if lams is not None:
        fm.lams = np.asarray(lams, dtype=np.float64)
    return fm


def integer_P(seed, n_orders, k, dn, da, density=0.3, keep=None):
    """integers in [-8, 8], mostly zero; dn rows of P[o].T are not all zero, at ids spread over da; rows 0 and 1 of the kept ones
    cancel exactly, (1, 1, 0 ..) against (1, -1, 0 ..), where k allows"""
    rng = np.random.RandomState(seed)
    keep = np.sort(rng.choice(da, dn, replace=False)) if keep is None else keep
    P = np.zeros((n_orders, k, da))
    for o in range(n_orders):
        rows = rng.randint(-8, 9, size=(dn, k)) * (rng.rand(dn, k) < density)
        rows[np.arange(dn), rng.randint(0, k, dn)] = rng.choice([-3, 1, 2, 8], dn)  # no kept row is all zero
        if k >= 2 and dn >= 2:
            rows[:2] = 0
            rows[0, :2], rows[1, :2] = (1, 1), (1, -1)
        P[o][:, keep] = rows.T
    return P


def check_exact(fm, order):
    want, pairs, weights = reference(fm, order, max(KS))  # (the K best are the first K of any longer ranking)
    assert fm.interactionStats(order) == want
    for K in KS:
        got_p, got_w = fm.topInteractions(K, order)
        assert np.array_equal(got_p, pairs[:K]) and got_w.tobytes() == weights[:K].tobytes(), K
    return want


@pytest.mark.parametrize("fitLower,order", (("explicit", 0), ("explicit", 1), ("augment", 0)))
@pytest.mark.parametrize("k", (1, 3, 33, 130))
@pytest.mark.parametrize("dn", (1, 2, T - 1, T, T + 1, 2 * T + 3))
def test_integers(dn, k, fitLower, order):
    n_orders = 2 if fitLower == "explicit" else 1
    da = 2 * dn + 5  # with the dummy feature of fitLower = augment among the rows
    fm = model(integer_P(dn * 1000 + k, n_orders, k, dn, da), fitLower)
    assert fm.P.shape[2] == da and (fm.nAugments == 1) == (fitLower == "augment")
    want = check_exact(fm, order)
    assert want["nNonzeroRows"] == dn
    assert nf.countInteractions(fm, order) == want["nInteractions"] and nf.countFeatures(fm, order) == want["nFeatures"]


def special(name):
    if name == "lams":
        return model(integer_P(1, 2, 5, T + 9, 2 * T + 30), lams=[2.0, -1.0, 0.0, 3.0, 1.0])
    if name == "block-sparse":  # groups of 2 T rows on factors of their own: most tiles are skipped by signature
        P = integer_P(2, 2, 12, 6 * T, 6 * T + 40, density=1.0)
        ids = np.flatnonzero((P[0] != 0).any(0))
        for g in range(3):
            P[:, :4 * g, ids[2 * T * g:2 * T * (g + 1)]] = 0
            P[:, 4 * (g + 1):, ids[2 * T * g:2 * T * (g + 1)]] = 0
        return model(P)
    if name == "grid-cap":  # more tiles than the launch has workgroups: a second trip of the tile walk
        nT = 1
        while nT * (nT + 1) // 2 <= N_CU * GRID_PER_CU:
            nT += 1
        return model(integer_P(3, 2, 3, nT * T - 5, nT * T + 11))
    return model(np.zeros((2, 4, 50)))  # "all-zero"


@pytest.mark.parametrize("name", ("lams", "block-sparse", "grid-cap", "all-zero"))
def test_integers_special(name):
    fm = special(name)
    want = check_exact(fm, 0)
    if name == "all-zero":
        assert want == {"l1Norm": 0.0, "l1OffDiag": 0.0, "nInteractions": 0, "nFeatures": 0, "nNonzeroRows": 0}
    if name == "block-sparse":
        assert want["nInteractions"] <= 3 * (2 * T) * (2 * T - 1) // 2


def gaussian_model():
    rng = np.random.RandomState(7)
    d, k = 3 * T + 5, 30
    group = rng.randint(0, 3, d)  # a feature's factors: ten of its group's, and the last five, shared by all
    mask = (np.arange(k)[None, :] // 10 == group[:, None]) | (np.arange(k)[None, :] >= 25)
    mask &= rng.rand(d, k) < 0.7
    mask[rng.rand(d) < 0.2] = False
    return model(np.stack([(rng.standard_normal((d, k)) * mask).T] * 2)), mask


def test_gaussian():
    fm, mask = gaussian_model()
    want, pairs, weights = reference(fm, 0, 256)
    W = (fm.P[0].T * fm.lams) @ fm.P[0]
    shared = (mask.astype(np.int64) @ mask.T) > 0
    assert np.all(W[~shared] == 0) and np.abs(W[shared]).min() > 1e-9  # every non-structural weight is far above rounding (1e-15)
    got = fm.interactionStats(0)
    for name in ("l1Norm", "l1OffDiag"):
        print("%s: |got - want| / bound = %.3g" % (name, abs(got[name] - want[name]) / (RTOL * want[name])))
        assert abs(got[name] - want[name]) <= RTOL * want[name]
    assert {n: got[n] for n in got if n[0] == "n"} == {n: want[n] for n in want if n[0] == "n"}
    got_p, got_w = fm.topInteractions(256, 0)
    print("weights: worst |got - want| / bound = %.3g" % (np.abs(got_w - weights) / (RTOL * np.abs(weights))).max())
    assert np.array_equal(got_p, pairs) and np.all(np.abs(got_w - weights) <= RTOL * np.abs(weights))


def test_reproducible():
    fm, _ = gaussian_model()
    first, (p1, w1) = fm.interactionStats(0), fm.topInteractions(100, 0)
    again, (p2, w2) = fm.interactionStats(0), fm.topInteractions(100, 0)
    assert np.array([first["l1Norm"], first["l1OffDiag"]]).tobytes() == np.array([again["l1Norm"], again["l1OffDiag"]]).tobytes() and first == again
    assert p1.tobytes() == p2.tobytes() and w1.tobytes() == w2.tobytes()
    dn, da = 2 * T + 3, 5 * T
    keeps = [np.sort(np.random.RandomState(s).choice(da, dn, replace=False)) for s in (0, 1)]
    a, b = (model(integer_P(11, 2, 7, dn, da, keep=keep)).interactionStats(0) for keep in keeps)
    assert a == b and a["nInteractions"] > 0


def test_refusals():
    L, ctx = capi.lib(), nf.default_context()
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=2)
    ffm.set_params(np.ones((3, 4, 2)), np.zeros(4), 0.0)
    cfm = nf.ConvexFactorizationMachine("r", maxComponents=2)
    cfm.set_params(np.ones((2, 6)), np.ones(2), np.zeros(6), 0.0)
    raw = nf.FactorizationMachine("r", nComponents=2)
    raw._d = 6
    fm = model(np.ones((2, 2, 6)))
    l1, counts, pairs, weights = np.zeros(2), np.zeros(3, dtype=np.int64), np.zeros((256, 2), dtype=np.int64), np.zeros(256)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for m, order, K, code, word in ((ffm, 0, 1, capi.ERR_UNSUPPORTED, "field-aware"), (cfm, 0, 1, capi.ERR_UNSUPPORTED, "Convex"),
                                    (raw, 0, 1, capi.ERR_NOT_FITTED, "not fitted"), (fm, 2, 1, capi.ERR_INVALID, "order"),
                                    (fm, -1, 1, capi.ERR_INVALID, "order"), (fm, 0, 0, capi.ERR_INVALID, "K = 0"), (fm, 0, 257, capi.ERR_INVALID, "K = 257")):
        h = m._push(ctx) if m.isInitialized else m._handle(ctx)
        if K == 1:
            assert L.nfm_model_interaction_stats(h, order, vp(l1), vp(counts)) == code and word in L.nfm_last_error().decode(), word
        assert L.nfm_model_top_interactions(h, order, K, vp(pairs), vp(weights)) == code and word in L.nfm_last_error().decode(), word
    with pytest.raises(ValueError, match="K = 257"):  # (the host raises the reference's ValueError for NFM_ERR_INVALID)
        fm.topInteractions(257)
