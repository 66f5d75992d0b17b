"""-m gpu: the mini-batch row phase (k_row_phase<L, SPLIT, OPT, GEN, MODE, SING>) and decisionFunction (k_fm_predict<L, SPLIT>,
k_fm_predict_orders<LT, SPLIT>) on every lane mapping, against the mini-batch oracle (oracle/nimfm_mb.c) and
O.fm_decision_function.

A launch of a few hundred samples gets the largest SPLIT of its L from choose_split, so every case here runs once per requested
slot count with NFM_SPLIT held for the whole fit (tests/row_slot_cases.py: the data, the table, and the restatement of which
kernel a request ends at; tests/test_row_slot_cases.py: that the table reaches all of them).  The oracle runs once per case and
every slot count is compared with it at the tolerances of tests/test_gpu_minibatch.py, tests/test_gpu_psgd.py and
tests/test_gpu_predict.py.

That the knob reached the launch is asserted, not assumed: nothing in these kernels is atomic, so two requests that the
restatement puts on the same kernels must give the same bits, and two that it puts on different slot counts must differ in at
least one bit -- the slots' partial sums are added in another order.  Which row kernel took each batch is asked as well: the
driver counts one route_row_* launch per batch (nfm_ctx_timing_get), and every fit's counts must be the restatement's."""
import collections
import math

import numpy as np
import pytest

import nimfm_amd as nf
import oracle as O
import row_slot_cases as R
from common import assert_close
from gpu_common import _env, gpu_fm, to_gpu
from test_gpu_col_long import assert_same_bits
from test_gpu_minibatch import run_oracle_sgd_mb
from test_gpu_psgd import REGS, make_stream
from test_gpu_psgd import run_oracle as run_oracle_psgd

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
EPOCHS = 2
# AdaGrad moves every touched parameter by about eta0 per step whatever the gradient's size: with rows of up to 150 entries the
# default 0.1 overshoots (the oracle's loss grows from 0.5 to 1e4 within two epochs at k = 50), and a run that diverges
# compares conditioning, not kernels
ADA_ETA0 = 0.01


def to_oracle(X):
    return O.Dataset(X.indptr, X.indices, X.data, X.n, X.d)


def start(X, k, model):
    degree, fit_lower, fit_linear = R.MODELS[model]
    nb, n_aug = R.n_orders(degree, fit_lower), R.n_augments(degree, fit_lower, fit_linear)
    rng = np.random.default_rng(k)
    P0 = rng.standard_normal((nb, k, X.d + n_aug)) * (0.1 / np.sqrt(k))
    w0 = rng.uniform(-0.1, 0.1, X.d) if fit_linear else np.zeros(X.d)
    return P0, w0, 0.05, nb, n_aug


def oracle_fit(group):
    """two epochs of the mini-batch rule on the CPU: P, w, b, it and the (viol, loss) history"""
    k, family, regime, solver, model = group
    X, y = R.train_data(family, regime)
    Xo = to_oracle(X)
    degree, fit_lower, fit_linear = R.MODELS[model]
    P0, w0, b0, nb, n_aug = start(X, k, model)
    batch = R.REGIMES[regime][1]
    perms = R.train_perms(family, regime)
    if solver == "sgd":
        P, w, b, it, hist = run_oracle_sgd_mb(Xo, y, degree, P0, w0, b0, O.sgd_cfg(fit_linear=fit_linear), batch, n_aug, perms, EPOCHS)
    else:
        cfg = O.adagrad_cfg(eta0=ADA_ETA0, fit_linear=fit_linear)
        P, w, b, it = P0.copy(), w0.copy(), b0, 1
        st = O.AdaState(nb, X.d + n_aug, k, X.d)
        hist = []
        for e in range(EPOCHS):
            b, it, ls, vs = O.fm_adagrad_epoch_mb(Xo, y, degree, P, w, b, cfg, batch, st, n_aug, perm=None if perms is None else perms[e], it=it)
            hist.append((vs, ls / X.n))
        b = O.fm_adagrad_finalize(degree, P, w, b, cfg, it, st, n_aug)
    assert np.isfinite(P).all() and np.isfinite(w).all() and np.isfinite(b)
    if nb:  # the interaction part is alive: AdaGrad starts from a zero state, and P = 0 is a fixed point of its rule
        touched = np.unique(X.indices)
        assert (P[:, :, touched] != 0.0).mean() > 0.95 and all(np.median(np.abs(P[o][:, touched])) > 1e-5 for o in range(nb))
    return {"P": P, "w": w, "b": b, "it": it, "viol": [h[0] for h in hist], "loss": [h[1] for h in hist]}


def gpu_fit(group, request, Xg, **env):
    """the same fit on the device with NFM_SPLIT=request, from a fresh optimizer: a captured epoch graph keeps its launches"""
    k, family, regime, solver, model = group
    X, y = R.train_data(family, regime)
    degree, fit_lower, fit_linear = R.MODELS[model]
    P0, w0, b0, nb, n_aug = start(X, k, model)
    perms = R.train_perms(family, regime)
    fm = gpu_fm("regression", degree, k, fit_lower, fit_linear, True, P0, w0, b0)
    kw = dict(maxIter=EPOCHS, verbose=0, tol=0, shuffle=perms is not None, mode="minibatch", batch=R.REGIMES[regime][1])
    opt = nf.newSGD(**kw) if solver == "sgd" else nf.newAdaGrad(eta0=ADA_ETA0, **kw)
    with _env(NFM_SPLIT=request, **env):
        if perms is None:
            opt.fit(Xg, y, fm)
        else:
            opt.fit(Xg, y, fm, perms=perms)
    return {"P": np.array(fm.P), "w": np.array(fm.w), "b": np.array([fm.intercept]), "it": opt.it,
            "viol": np.array([h[0] for h in opt.history]), "loss": np.array([h[1] for h in opt.history])}


ROW_COUNTERS = ["route_row_m%d" % m for m in range(5)] + ["route_row_ada2"]


def row_counts(ctx):
    return np.array([ctx.timing_get(name)[0] for name in ROW_COUNTERS])


def restated_row_counts(case):
    """batches per row kernel of the fit, from R.fit_paths (its MODE 2 is MODE 2 here: the tables are far below 384 MB)"""
    c = collections.Counter("route_row_ada2" if p.kernel == "ada2" else "route_row_m%d" % p.mode for p in R.fit_paths(case))
    return np.array([c[name] for name in ROW_COUNTERS])


def bits(res):
    return {key: np.ascontiguousarray(res[key], dtype=np.float64) for key in ("P", "w", "b", "viol", "loss")}


def differs(a, b, key):
    return bool((np.asarray(a[key]).view(np.uint64) != np.asarray(b[key]).view(np.uint64)).any())


def check_signatures(results, sig_of, key, what):
    """results: request -> arrays; sig_of: request -> what of the request reaches the result according to the restatement"""
    reqs = list(results)
    for i, qa in enumerate(reqs):
        for qb in reqs[i + 1:]:
            if sig_of[qa] == sig_of[qb]:
                assert_same_bits(bits(results[qa]), bits(results[qb]), "%s: NFM_SPLIT=%d and %d end at the same kernels" % (what, qa, qb))
            else:  # another slot count adds a sample's partial sums in another order
                assert differs(results[qa], results[qb], key), "%s: NFM_SPLIT=%d and %d give the same %s bit for bit" % (what, qa, qb, key)


TRAIN_GROUPS = [g for g in R.groups() if g[3] != "mbpsgd"]


@pytest.mark.parametrize("group", TRAIN_GROUPS, ids=lambda g: "-".join(str(v) for v in g))
def test_row_phase_at_every_slot_count(group):
    k, family, regime, solver, model = group
    X, y = R.train_data(family, regime)
    ref = oracle_fit(group)
    Xg = to_gpu(to_oracle(X))
    results, sig_of = {}, {}
    for case in R.cases_of(group):
        n0 = row_counts(Xg.ctx)
        got = gpu_fit(group, case.request, Xg)
        what = "NFM_SPLIT=%d (SPLIT %d)" % (case.request, R.row_slots(R.lanes_for_k(k), case.request))
        assert (row_counts(Xg.ctx) - n0).tolist() == restated_row_counts(case).tolist(), what + " " + str(ROW_COUNTERS)
        assert got["it"] == ref["it"]
        assert abs(got["b"][0] - ref["b"]) < 1e-11, what
        assert_close(got["w"], ref["w"], RTOL, ATOL, what + " w")
        assert_close(got["P"], ref["P"], RTOL, ATOL, what + " P")
        assert_close(got["loss"], ref["loss"], 1e-10, 1e-13, what + " loss")
        assert_close(got["viol"], ref["viol"], 1e-9, 1e-12, what + " viol")
        results[case.request], sig_of[case.request] = got, R.signature(case)
    # a model of degree 1 has no P: its linear term is what the slots add up
    check_signatures(results, sig_of, "w" if model == "deg1" else "P", "-".join(str(v) for v in group))


def test_mbpsgd_row_phase_at_every_slot_count():
    """MBPSGD's forward pass is AdaGrad's row phase reading the stored parameters (use_stored); rows of up to 150 entries at
    k = 13: MODE 3 with chunks of 32 and of 64 held entries.  The oracle, the stream and the tolerances of test_gpu_psgd.py."""
    group = R.groups()[-1]
    k, family, regime, solver, model = group
    assert solver == "mbpsgd"
    X, y = R.train_data(family, regime)
    Xo = to_oracle(X)
    degree, fit_lower, fit_linear = R.MODELS[model]
    P0, w0, b0, nb, n_aug = start(X, k, model)
    B, outer = R.REGIMES[regime][1], 2
    inner = (X.n - 1) // B + 1
    stream = make_stream(X.n, B * inner * outer, 9)
    cfg = O.psgd_cfg(eta0=1.0, gamma=2e-3, beta=1e-2, alpha=1e-2, alpha0=1e-2, reg="l1")
    P, w, b, it, losses = run_oracle_psgd(Xo, y, degree, P0, w0, b0, cfg, stream, B, inner, outer, n_aug)
    assert np.isfinite(P).all() and 0.05 < (P == 0.0).mean() < 0.95  # steps of the size of P itself, and the prox bites
    Xg = to_gpu(Xo)
    results, sig_of = {}, {}
    for case in R.cases_of(group):
        fm = gpu_fm("regression", degree, k, fit_lower, fit_linear, True, P0, w0, b0)
        opt = nf.newMBPSGD(maxIter=outer, eta0=1.0, alpha0=1e-2, alpha=1e-2, beta=1e-2, gamma=2e-3, reg=REGS["l1"](), miniBatchSize=B,
                           verbose=0, tol=-1.0)
        opt.it = 1
        n0 = row_counts(Xg.ctx)
        with _env(NFM_SPLIT=case.request):
            opt.fit(Xg, y, fm, stream=stream)
        what = "NFM_SPLIT=%d" % case.request
        assert (row_counts(Xg.ctx) - n0).tolist() == restated_row_counts(case).tolist(), what + " " + str(ROW_COUNTERS)
        assert opt.it == it
        assert_close([h[1] for h in opt.history], losses, 1e-10, 1e-13, what + " running loss")
        assert abs(fm.intercept - b) < 1e-10
        assert_close(fm.w, w, RTOL, ATOL, what + " w")
        assert_close(fm.P, P, RTOL, ATOL, what + " P")
        results[case.request] = {"P": np.array(fm.P), "w": np.array(fm.w), "b": np.array([fm.intercept]),
                                 "viol": np.zeros(1), "loss": np.array([h[1] for h in opt.history])}
        sig_of[case.request] = R.signature(case)
    assert [p.mode for p in R.fit_paths(R.cases_of(group)[0])] == [3] * (inner * outer)
    check_signatures(results, sig_of, "P", "mbpsgd")


def test_staged_linear_weights_at_a_stride_of_32():
    """k_stage_w writes Wt[pib * CAP + q] and k_row_phase<.., MODE 1> reads it back with its own CAP = E * L * SPLIT: 32 at
    k = 13 with one slot, 64 with two.  Staged against gathered bit for bit, and both against the oracle."""
    group = (13, "short", "dense", "sgd", "deg2")
    assert [R.stage_w_cap(R.Case(13, q, *group[1:])) for q in (1, 2)] == [32, 64]
    X, y = R.train_data("short", "dense")
    ref = oracle_fit(group)
    Xg = to_gpu(to_oracle(X))
    for request in (1, 2):
        n0, r0 = Xg.ctx.timing_get("stage_w")[0], row_counts(Xg.ctx)
        on = gpu_fit(group, request, Xg, NFM_STAGE_W=1)
        n1, r1 = Xg.ctx.timing_get("stage_w")[0], row_counts(Xg.ctx)
        off = gpu_fit(group, request, Xg, NFM_STAGE_W=0)
        want = restated_row_counts(R.Case(13, request, *group[1:])).tolist()
        assert (r1 - r0).tolist() == want == (row_counts(Xg.ctx) - r1).tolist() and want[1] == sum(want)  # MODE 1, staged or not
        assert n1 > n0 and Xg.ctx.timing_get("stage_w")[0] == n1, "stage_w launches: %d with NFM_STAGE_W=1" % (n1 - n0)
        assert_same_bits(bits(on), bits(off), "NFM_SPLIT=%d: staged vs gathered" % request)
        assert abs(on["b"][0] - ref["b"]) < 1e-11
        assert_close(on["w"], ref["w"], RTOL, ATOL, "w")
        assert_close(on["P"], ref["P"], RTOL, ATOL, "P")


# ---------------------------------------------------------------- decisionFunction
def slow_rows(X, degree, P, w, b, n_aug, lams, k):
    """the brute-force definition (O.slow_fm_decision_function) on the rows where it is affordable: it walks every combination
    of `degree` features, so a row is taken alone with its own entries and the dummy features as the feature space (absent
    features add nothing), as long as that is at most 3e5 products per order.  lams[s] * K_t(p, x) = K_t(lams[s]^(1/t) p, x): the
    ANOVA kernel of degree t is homogeneous of degree t in p, and the brute force takes no lams."""
    Ps = np.stack([P[o] * (lams ** (1.0 / (degree - o)))[:, None] for o in range(P.shape[0])]) if P.shape[0] else P
    rows, out = [], []
    for i in range(X.n):
        q0, q1 = int(X.indptr[i]), int(X.indptr[i + 1])
        m = q1 - q0
        if m == 0 or math.comb(m + n_aug, degree) * k > 3e5:
            continue
        cols = X.indices[q0:q1]
        sub = np.concatenate([cols, X.d + np.arange(n_aug, dtype=np.int64)])
        rows.append(i)
        out.append(O.slow_fm_decision_function(np.array(X.data[q0:q1])[None, :], degree, Ps[:, :, sub], w[cols], b, n_aug)[0])
    return np.array(rows), np.array(out)


@pytest.mark.parametrize("model", list(R.PREDICT_MODELS))
@pytest.mark.parametrize("k", R.KS)
def test_decision_function_at_every_slot_count(k, model):
    X = R.predict_data()
    Xo = to_oracle(X)
    degree, fit_lower = R.PREDICT_MODELS[model]
    nb, n_aug = R.n_orders(degree, fit_lower), R.n_augments(degree, fit_lower, True)
    rng = np.random.default_rng(100 * k + degree)
    P = rng.standard_normal((nb, k, X.d + n_aug)) * 0.2
    w, b, lams = rng.standard_normal(X.d), -1.5, rng.uniform(0.5, 1.5, size=k)
    want = O.fm_decision_function(Xo, degree, P, w, b, n_aug, lams=lams)
    rows, slow = slow_rows(X, degree, P, w, b, n_aug, lams, k)
    assert len(rows) >= X.n // 3 and X.lengths()[rows].max() >= 16
    assert_close(want[rows], slow, 1e-6, 1e-9, "oracle vs brute force")
    fm = gpu_fm("regression", degree, k, fit_lower, True, True, P, w, b)
    fm.lams = lams
    fm.set_params(P, w, b)
    Xg = to_gpu(Xo)
    results, sig_of = {}, {}
    for request in R.requests(R.lanes_for_k(k)):
        with _env(NFM_SPLIT=request):
            got = np.array(fm.decisionFunction(Xg), dtype=np.float64)
        sig_of[request] = R.predict_kernel(k, request, model, X)
        what = "NFM_SPLIT=%d %s" % (request, sig_of[request])
        assert_close(got, want, 1e-10, 1e-12, what)
        assert_close(got[rows], slow, 1e-6, 1e-9, what + " vs brute force")
        results[request] = got
    reqs = list(results)
    for i, qa in enumerate(reqs):
        for qb in reqs[i + 1:]:
            same = np.array_equal(results[qa].view(np.uint64), results[qb].view(np.uint64))
            if sig_of[qa] == sig_of[qb]:  # the same instance: k_fm_predict_orders<64, 1> at every request, or a clamped request
                assert same, "NFM_SPLIT=%d and %d both end at %s" % (qa, qb, sig_of[qa])
            else:
                assert not same, "NFM_SPLIT=%d (%s) and %d (%s) predict the same bits" % (qa, sig_of[qa], qb, sig_of[qb])
