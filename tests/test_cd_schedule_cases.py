"""CPU: the conditions the inputs of tests/cd_schedule_cases.py must meet so that the schedule-edge tests of
tests/test_gpu_cd.py, tests/test_gpu_pcd.py and tests/test_gpu_pbcd.py reach the code they are there for and may keep the
tolerances of their files.  No GPU: the restatements only.

Coverage is asserted, not claimed: kWave, kBlock, kWideMin and kNarrowBlock are read out of common.h and cd_dev.h, and the
sequence of launches sweep_levels and sweep_runs would issue, the widths and the column lengths are recomputed from the
restatements' schedules, so a later retune of a constant fails here instead of silently ending the coverage.

Spread of the restatements between sequential and pairwise sums over every sample (the intercept's, the dummy features' and
the loss's: the sums the device takes with a fixed tree), measured here as max |dP| / max |P|, |dw|, |db| and the relative
distance of viol and the mean loss, over the 20 cases below that the GPU tests compare with a tolerance: at most 2.9e-14
(edges, PCD with L1 at degree 3, intercept and logistic loss); 1.6e-14 on edges_gaps (column-wise SquaredL12), 9.0e-15 on
long_1025 (PBCD with L21 at degree 3, augment, k = 5).  All are below 1e-11, a tenth of RTOL = 1e-10 of the three GPU files, so
no tolerance is widened and no case shrunk."""
import os
import re

import numpy as np
import pytest

import cd_restatement as C
import cd_schedule_cases as S
import pbcd_restatement as B
import pcd_restatement as Pc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")


def _const(name, file):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


kWave, kBlock = _const("kWave", "common.h"), _const("kBlock", "common.h")
kWideMin, kNarrowBlock = _const("kWideMin", "cd_dev.h"), _const("kNarrowBlock", "cd_dev.h")
kWavesPerBlock, kNarrowWaves = kBlock // kWave, kNarrowBlock // kWave


def test_the_source_still_has_the_branches_these_numbers_describe():
    common, dev, cd, pb = (open(os.path.join(CSRC, f)).read() for f in ("common.h", "cd_dev.h", "cd.hip", "pbcd.hip"))
    assert "constexpr int kWavesPerBlock = kBlock / kWave;" in common
    assert "constexpr int kNarrowWaves = kNarrowBlock / kWave;" in dev
    for text in (cd, pb):
        assert text.count("width >= kWideMin") == 2  # the level sweep and the run sweep
        assert "f += kNarrowWaves" in text
        assert "< kWideMin) ++g1;" in text and "< kWideMin) ++r1;" in text
    assert "j += kNarrowWaves" in pb  # k_pb_sq_runs
    assert "base += kWave" in cd and "q += kWave" in cd  # cd_grad, cd_sync
    assert "base += kNarrowBlock" in cd  # k_pcd_chain
    assert "__shared__ double su[kWideMin], si[kWideMin], sp[kWideMin], sd[kWideMin];" in cd  # k_pcd_runs
    assert "i += kNarrowBlock" in cd and "i += kNarrowBlock" in pb  # the sums over every sample
    assert "B.nc <= kWave / 2" in pb and "sb += kWave" in pb
    assert 'getenv("NFM_CD_GRAPH")' in cd


def schedules(name):
    """(level widths, run widths, column lengths) from the restatements"""
    Xo, _ = S.inputs(name)
    cols = C.columns(Xo.indptr, Xo.indices, Xo.data, Xo.n, Xo.d)
    lv = C.levels(cols, Xo.n)
    return [lv.count(v) for v in sorted(set(lv))], [len(r) for r in Pc.runs(cols)], [len(c) for c in cols]


def check_launches(seq):
    """at least two one-workgroup walks, one of them behind a wide launch and ahead of another (wide -> narrow -> wide), and a
    walk of several levels (runs)"""
    kinds = [k for k, _ in seq]
    narrow = [i for i, k in enumerate(kinds) if k == "narrow"]
    assert len(narrow) >= 2 and any(i > 0 for i in narrow)
    assert any(0 < i < len(kinds) - 1 for i in narrow)
    assert any(len(w) > 1 for k, w in seq if k == "narrow")
    assert all(kinds[i] != kinds[i + 1] or kinds[i] == "wide" for i in range(len(kinds) - 1))


def test_builder_is_banded_one_hot():
    for name, c in S.CASES.items():
        Xo, y = S.inputs(name)
        m = len(c["groups"])
        assert Xo.n == c["n"] and len(Xo.data) == Xo.n * m and np.all(np.diff(Xo.indptr) == m)
        rows = Xo.indices.reshape(Xo.n, m)
        assert np.all(np.diff(rows, axis=1) > 0)  # sorted rows, no repeated id
        for g, ids in enumerate(S.group_ids(name)):
            assert np.all(np.isin(rows[:, g], ids))
            assert [int((rows[:, g] == j).sum()) for j in ids] == S.counts_of(c["groups"][g], Xo.n)
        a = np.abs(Xo.data)
        assert a.min() >= 0.5 and a.max() <= 1.5 and (Xo.data < 0).any() and (Xo.data > 0).any()
        empties = S.empty_columns(name)
        if c.get("gaps"):
            assert len(empties) == sum(len(i) for i in S.group_ids(name)) + sum(c["pad"]) and c["pad"][-1] == 3
            assert Xo.d == 657
        else:
            assert len(empties) == 0
    assert S.inputs("edges")[0].d == 376 and len(S.inputs("edges")[0].data) == 2898
    assert S.inputs("long_1025")[0].d == 1093


def test_edges_reaches_every_width_and_length_edge():
    lw, rw, lens = schedules("edges")
    assert lw == rw == [63, 64, 65, 1, 16, 17, 15, 130, 5]  # group g is level g + 1 and run g
    Xo, _ = S.inputs("edges")
    assert C.schedule_depth(Xo.indptr, Xo.indices, Xo.n, Xo.d) == Pc.schedule(Xo.indptr, Xo.indices, Xo.n, Xo.d, True) == (9, 130)
    seq = S.launches(lw, kWideMin)
    assert seq == [("narrow", [63]), ("wide", 64), ("wide", 65), ("narrow", [1, 16, 17, 15]), ("wide", 130), ("narrow", [5])]
    check_launches(seq)
    widths = set(lw)
    assert {kWideMin - 1, kWideMin, kWideMin + 1} <= widths  # either side of the cut, and k_pcd_runs' LDS arrays full but one
    assert {kNarrowWaves - 1, kNarrowWaves, kNarrowWaves + 1, 1} <= widths  # f += kNarrowWaves: its second trip at 17
    wide = [w for w in lw if w >= kWideMin]
    assert any(w % kWavesPerBlock for w in wide) and any(w % kWavesPerBlock == 0 for w in wide)  # a partial last workgroup
    assert max(wide) > 2 * kWideMin
    last = [lens[j] for j in S.group_ids("edges")[-1]]
    assert last == [kWave - 1, kWave, kWave + 1, 1, 2 * kWave + 1]  # cd_grad's partial cnt, cd_sync's q += kWave
    every = lens[int(S.group_ids("edges")[3][0])]
    assert every == Xo.n == 322 and every // kWave == 5 and every % kWave  # five full chunks and a partial one


def test_edges_gaps_keeps_the_edges_behind_empty_columns():
    lw, rw, lens = schedules("edges_gaps")
    Xo, _ = S.inputs("edges_gaps")
    empties = S.empty_columns("edges_gaps")
    used = np.concatenate(S.group_ids("edges_gaps"))
    assert np.all(np.isin(used + 1, empties)) and np.all(np.isin(np.arange(Xo.d - 3, Xo.d), empties))  # a gap behind every feature
    assert lw[0] == len(empties) == 331 >= kWideMin  # level 0: every empty column, a wide launch of skipped (clamped) steps
    assert lw[1:] == [31, 32, 32, 1, 16, 17, 63, 64, 65, 5]
    assert rw == [63, 64, 65, 2, 32, 34, 126, 128, 130, 13]
    assert {kWideMin - 1, kWideMin, kWideMin + 1} <= set(rw) and {kWideMin - 1, kWideMin, kWideMin + 1} <= set(lw)
    lseq, rseq = S.launches(lw, kWideMin), S.launches(rw, kWideMin)
    assert lseq == [("wide", 331), ("narrow", [31, 32, 32, 1, 16, 17, 63]), ("wide", 64), ("wide", 65), ("narrow", [5])]
    assert rseq == [("narrow", [63]), ("wide", 64), ("wide", 65), ("narrow", [2, 32, 34]), ("wide", 126), ("wide", 128),
                    ("wide", 130), ("narrow", [13])]
    check_launches(lseq)
    check_launches(rseq)
    # skipped steps in both kinds of launch: empty columns inside narrow runs (k_pcd_runs) and inside wide ones (k_pcd_chain, k_pcd_sync)
    runs = Pc.runs(C.columns(Xo.indptr, Xo.indices, Xo.data, Xo.n, Xo.d))
    for r in runs:
        assert any(lens[j] == 0 for j in r) and any(lens[j] > 0 for j in r)
    assert {lens[j] for j in S.group_ids("edges_gaps")[-1]} == {kWave - 1, kWave, kWave + 1, 1, 2 * kWave + 1}


@pytest.mark.parametrize("name,first", [("long_1025", 1025), ("long_1024", 1024)])
def test_long_reaches_the_second_trips(name, first):
    lw, rw, lens = schedules(name)
    Xo, _ = S.inputs(name)
    assert lw == rw == [first, 1, 64, 3]
    assert first == kNarrowBlock + (name == "long_1025")  # k_pcd_chain: one full LDS chunk, and one more feature
    assert Xo.n == 2 * kNarrowBlock + 2  # block_sum's callers: two full trips of i += kNarrowBlock and a partial one
    seq = S.launches(rw, kWideMin)
    assert [k for k, _ in seq] == ["wide", "narrow", "wide", "narrow"]
    assert max(lens) == Xo.n  # the width-1 group: 32 full chunks and a partial one
    assert Xo.n // kWave == 32 and Xo.n % kWave == 2


def test_pbcd_components_reach_both_layouts():
    """pb_grad: nc <= kWave / 2 packs 64 / w samples of w lanes each, above that one lane per component in blocks of kWave"""
    def w_of(k):
        w = 1
        while w < k:
            w <<= 1
        return w
    half = kWave // 2
    assert S.PBCD_K == (3, 5, half, half + 1, kWave, kWave + 1)
    assert w_of(3) == 4 and w_of(5) == 8 and w_of(half) == half and kWave // w_of(half) == 2
    lens = set(schedules("edges")[2])
    for k in (3, 5, half):  # column lengths either side of a multiple of the samples in flight, and below one slot set
        per = kWave // w_of(k)
        assert any(n % per == 0 for n in lens) and any(n % per == 1 for n in lens) and any(n % per == per - 1 for n in lens), k
        assert any(n < per for n in lens) or per == 2


# ---------------------------------------------------------------- the conditions of the comparison, on the restatements
PCD_RE = {"l1": ("l1", False), "sq_row": ("squaredl12", False), "sq_col": ("squaredl12", True), "ti": ("omegati", False)}


def restate(name, solver, reg, degree=2, k=4, fit_lower="explicit", fit_linear=True, fit_intercept=False, **kw):
    Xo, y = S.inputs(name)
    P0, w0, b0, n_aug = S.start(Xo, degree, k, fit_lower, fit_linear, fit_intercept)
    args = (Xo.indptr, Xo.indices, Xo.data, y, P0, w0, b0, degree, n_aug, fit_linear, fit_intercept)
    kw = dict(dict(tol=0.0, maxIter=3), **kw)
    if solver == "cd":
        return C.fit(*args, **kw), P0
    gamma = kw.pop("gamma", None) or S.gamma_of(name, reg)
    if solver == "pcd":
        rn, tr = PCD_RE[reg]
        return Pc.fit(*args, reg=rn, transpose=tr, gamma=gamma, **kw), P0
    return B.fit(*args, reg=reg, gamma=gamma, **kw), P0


def zero_share(name, P):
    used = np.ones(P.shape[2], dtype=bool)
    used[S.empty_columns(name)] = False
    used[S.inputs(name)[0].d:] = False  # dummy features apart, too
    return float((P[:, :, used] == 0.0).mean())


GAPS_KW = dict(beta=0.0, alpha=0.0)
SHARES = [(n, "pcd", r, kw) for n, kw in (("edges", {}), ("edges_gaps", GAPS_KW), ("long_1025", dict(maxIter=2)),
                                          ("long_1024", dict(maxIter=2))) for r in PCD_RE]
SHARES += [(n, "pbcd", r, kw) for n, kw in (("edges", {}), ("edges_gaps", GAPS_KW), ("long_1025", dict(maxIter=2)))
           for r in ("l1", "l21", "squaredl21")]


@pytest.mark.parametrize("name,solver,reg,kw", SHARES, ids=lambda v: v if isinstance(v, str) else "kw")
def test_the_prox_zeroes_some_and_not_all(name, solver, reg, kw):
    (P, w, b, hist, _), P0 = restate(name, solver, reg, **kw)
    share = zero_share(name, P)
    print("%s %s %s zeros %.3f" % (name, solver, reg, share))
    assert 0.05 < share < 0.95, (name, solver, reg, share)
    assert np.isfinite(P).all() and np.isfinite(w).all() and np.isfinite(np.array(hist)).all()
    if name == "edges_gaps":
        e = S.empty_columns(name)
        if solver == "pcd":  # a skipped step: neither the prox nor the cache hook, P bit-unchanged
            assert np.array_equal(P[:, :, e], P0[:, :, e])
        else:  # the clamp inv = 1e-12: lam = gamma / 1e-12, finite, and the prox moves the row (to zero)
            assert np.isfinite(P[:, :, e]).all() and np.all(P[:, :, e] == 0.0) and np.all(P0[:, :, e] != 0.0)


@pytest.mark.parametrize("k", S.PBCD_K)
@pytest.mark.parametrize("reg", ["l21", "squaredl21"])
def test_pbcd_component_cases_zero_some_rows(reg, k):
    (P, _, _, _, _), _ = restate("edges", "pbcd", reg, k=k, maxIter=3, gamma=S.PBCD_K_GAMMA[reg][k])
    share = zero_share("edges", P)
    print("edges pbcd %s k %d zeros %.3f" % (reg, k, share))
    assert 0.05 < share < 0.95, (reg, k, share)


# the cases the GPU tests compare at RTOL: (case, solver, regulariser, keywords of restate)
LOGISTIC = dict(fit_intercept=True, loss="logistic", task="classification")
LONG = dict(fit_lower="augment", maxIter=2, **LOGISTIC)
TOLERANCE_CASES = [("edges", "cd", None, dict(degree=3, **LOGISTIC)), ("long_1025", "cd", None, dict(degree=3, **LONG))]
TOLERANCE_CASES += [("edges", "pcd", r, dict(degree=2 if r.startswith("sq") else 3, **LOGISTIC)) for r in PCD_RE]
TOLERANCE_CASES += [("edges_gaps", "pcd", r, dict(fit_intercept=True, **GAPS_KW)) for r in PCD_RE]
TOLERANCE_CASES += [("long_1025", "pcd", r, dict(degree=3, **LONG)) for r in ("l1", "ti")]
TOLERANCE_CASES += [("edges", "pbcd", r, dict(degree=2 if r == "squaredl21" else 3, **LOGISTIC)) for r in ("l1", "l21", "squaredl21")]
TOLERANCE_CASES += [("edges_gaps", "pbcd", r, dict(fit_intercept=True, **GAPS_KW)) for r in ("l1", "l21", "squaredl21")]
TOLERANCE_CASES += [("long_1025", "pbcd", "squaredl21", dict(k=5, fit_intercept=True, maxIter=2)),
                    ("long_1025", "pbcd", "l21", dict(degree=3, k=5, fit_lower="augment", fit_intercept=True, maxIter=2))]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300))) if a.size else 0.0


@pytest.mark.parametrize("name,solver,reg,kw", TOLERANCE_CASES, ids=lambda v: v if isinstance(v, str) else "kw")
def test_spread_between_sequential_and_pairwise_sums(name, solver, reg, kw):
    (P, w, b, hist, _), _ = restate(name, solver, reg, **kw)
    (P2, w2, b2, hist2, _), _ = restate(name, solver, reg, sums="pair", **kw)
    spread = max(np.abs(P - P2).max() / np.abs(P).max(), np.abs(w - w2).max(), abs(b - b2), rel(hist, hist2))
    print("spread %-10s %-5s %-10s %.3e" % (name, solver, reg, spread))
    assert spread > 0.0 or not kw.get("fit_intercept")  # the switch is live: the two orders differ somewhere
    assert spread <= 1e-11, (name, solver, reg, spread)  # a tenth of RTOL = 1e-10
    assert np.array_equal(P == 0.0, P2 == 0.0)
