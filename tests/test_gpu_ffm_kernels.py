"""-m gpu: the field-aware mini-batch kernels (csrc/mb_ffm.hip) and k_ffm_predict (csrc/predict.hip) at every lane width
L = 1 .. 64 and under every choice run_ffm makes per fit -- the generic row kernel, the LDS-resident one with one sample per
wavefront and with one per workgroup, dynamic LDS on both sides of 64 KiB, the heavy column path at exactly 128 and 129 touches,
k_ffm_refresh -- against the mini-batch oracle (oracle/nimfm_mb.c) and O.ffm_decision_function.

Which kernel ran is asserted, not assumed: run_ffm counts every row-phase launch under "ffm_row_generic", "ffm_row_lds" or
"ffm_row_coop" and, with more than 64 KiB of dynamic LDS, under "ffm_row_lds_big"; the counters are read before and after
every fit and compared with the restatement of the host's choice in tests/ffm_kernel_cases.py (the data, the table and the
restatement; tests/test_ffm_kernel_cases.py: that the table reaches everything, and that the oracle's fits are worth comparing
with).  Tolerances are those of tests/test_gpu_minibatch.py for field-aware models and of tests/test_gpu_predict.py.  Run with
-s to see the counters of every case."""
import numpy as np
import pytest

import ffm_kernel_cases as K
import nimfm_amd as nf
import oracle as O
from common import assert_close, make_ffm_dataset
from gpu_common import gpu_ffm, to_gpu
from test_ffm_kernel_cases import assert_usable, oracle_fit, to_oracle
from test_gpu_col_long import assert_same_bits

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
COUNTED = tuple(K.FAMILY.values()) + (K.BIG, "row_phase", "refresh", "heavy_partial", "heavy_apply")


def counters(ctx):
    return {f: ctx.timing_get(f)[0] for f in COUNTED}


def optimizer(solver, batch, cap=1.0, shuffle=False):
    kw = dict(maxIter=K.EPOCHS, verbose=0, tol=0, shuffle=shuffle, mode="minibatch", batch=batch)
    return nf.newSGD(eta0=K.SGD_ETA0, touchCap=cap, **kw) if solver == "sgd" else nf.newAdaGrad(eta0=K.ADA_ETA0, **kw)


def read_back(ffm, opt, solver, viol, loss):
    out = {"P": np.array(ffm.P), "w": np.array(ffm.w), "b": np.array([ffm.intercept]), "it": opt.it,
           "viol": np.array(viol, dtype=np.float64), "loss": np.array(loss, dtype=np.float64)}
    if solver == "adagrad":
        gs, gn, gsw, gnw, gsb, gnb = opt.get_state(ffm)
        out.update(g_sum=np.array(gs), g_norm=np.array(gn))
    return out


def gpu_fit(X, Xg, y, k, solver, batch, perms=None, fit_linear=True, fit_intercept=True, cap=1.0, timing=False):
    """the fit of oracle_fit on the device, from a fresh model and optimizer -> (what it left, launches per counted family)"""
    P0, w0, b0 = K.start(X.d, X.F, k, fit_linear)
    ffm = gpu_ffm("regression", k, fit_linear, fit_intercept, P0, w0, b0)
    opt = optimizer(solver, batch, cap, perms is not None)
    ctx = Xg.ctx
    before = counters(ctx)
    if timing:  # the families TimedLaunch counts: "row_phase", "refresh", "heavy_partial", "heavy_apply"
        ctx.timing_enable(True)
    try:
        if perms is None:
            opt.fit(Xg, y, ffm)
        else:
            opt.fit(Xg, y, ffm, perms=perms)
        after = counters(ctx)
    finally:
        if timing:
            ctx.timing_enable(False)
    got = read_back(ffm, opt, solver, [h[0] for h in opt.history], [h[1] for h in opt.history])
    return got, {f: after[f] - before[f] for f in COUNTED}


def compare(got, ref, solver, what):
    assert got["it"] == ref["it"], what
    assert abs(got["b"][0] - ref["b"]) < 1e-11, what
    assert_close(got["w"], ref["w"], RTOL, ATOL, what + " w")
    assert_close(got["P"], ref["P"], RTOL, ATOL, what + " P")
    assert_close(got["loss"], ref["loss"], 1e-10, 1e-13, what + " loss")
    assert_close(got["viol"], ref["viol"], 1e-9, 1e-12, what + " viol")
    if solver == "adagrad":
        assert_close(got["g_sum"], ref["g_sum"], 1e-9, 1e-13, what + " g_sum")
        assert_close(got["g_norm"], ref["g_norm"], 1e-9, 1e-16, what + " g_norm")


def check_row_counters(n, case, solver, what, timed=False):
    """all row-phase launches of the fit under the family of the kernel the restatement names, and under no other"""
    launches = K.row_launches(solver)
    want = {f: 0 for f in COUNTED}
    want[K.FAMILY[case.kernel]] = launches
    want[K.BIG] = launches if case.lds_bytes > K.LDS_DEFAULT else 0
    print("%s: %s" % (what, ", ".join("%s %d" % (f, n[f]) for f in COUNTED)))
    for f in tuple(K.FAMILY.values()) + (K.BIG,):
        assert n[f] == want[f], "%s: %d launches counted under %s, %d expected (%s, %d B of dynamic LDS)" % (
            what, n[f], f, want[f], case.kernel, case.lds_bytes)
    if timed:
        assert n["row_phase"] == launches
    else:  # with timing off TimedLaunch counts nothing: the new counters do not depend on it
        assert n["row_phase"] == 0


# ---------------------------------------------------------------- the row kernels
@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
@pytest.mark.parametrize("case", K.ROW_CASES, ids=lambda c: c.name)
def test_row_kernels_at_every_lane_width(case, solver):
    X, y = K.row_data(case.name)
    perms = K.row_perms()
    ref = oracle_fit(X, y, case.k, solver, K.BATCH, perms)
    what = "%s %s" % (case.name, solver)
    assert_usable(ref, what)
    got, n = gpu_fit(X, to_gpu(to_oracle(X)), y, case.k, solver, K.BATCH, perms)
    check_row_counters(n, case, solver, what)
    compare(got, ref, solver, what)


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
@pytest.mark.parametrize("flags", K.FLAGS, ids=lambda f: "lin%d_b%d" % f)
@pytest.mark.parametrize("name", K.FLAG_CASES)
def test_row_kernels_with_every_model_flag(name, flags, solver):
    case = K.ROW_BY_NAME[name]
    X, y = K.row_data(name)
    perms = K.row_perms()
    ref = oracle_fit(X, y, case.k, solver, K.BATCH, perms, *flags)
    what = "%s lin%d b%d %s" % ((name,) + flags + (solver,))
    got, n = gpu_fit(X, to_gpu(to_oracle(X)), y, case.k, solver, K.BATCH, perms, *flags, timing=True)
    check_row_counters(n, case, solver, what, timed=True)
    compare(got, ref, solver, what)
    P0, w0, b0 = K.start(X.d, X.F, case.k, flags[0])
    assert flags[0] or (got["w"] == 0.0).all()
    assert flags[1] or got["b"][0] == b0


def epochs_over_the_first_rows(X, y, k, solver, perms, n_fit):
    """EPOCHS calls of nfm_opt_epoch over the positions [0, n_fit) of perms, on a data set that may hold more rows"""
    Xg = to_gpu(to_oracle(X))
    Xg.set_targets(np.ascontiguousarray(y, dtype=np.float64))
    P0, w0, b0 = K.start(X.d, X.F, k)
    ffm = gpu_ffm("regression", k, True, True, P0, w0, b0)
    opt = optimizer(solver, K.BATCH, shuffle=True)
    opt._handle(ffm, Xg.ctx, "minibatch")
    before = counters(Xg.ctx)
    viol, loss = [], []
    for e in range(K.EPOCHS):
        ls, vs = opt._epoch(Xg, np.ascontiguousarray(perms[e], dtype=np.int64), 0, n_fit)
        opt.it += n_fit
        viol.append(vs)
        loss.append(ls / n_fit)
    opt._finalize_into(ffm)
    after = counters(Xg.ctx)
    return read_back(ffm, opt, solver, viol, loss), {f: after[f] - before[f] for f in COUNTED}


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
def test_lds_and_generic_row_kernels_give_the_same_bits(solver):
    """On rows of at most 64 entries k_ffm_row_phase_lds<.., 4, false> and k_ffm_row_phase deal the outputs (q, f) to the lane
    groups alike (o = ob + g), add a row's partners in ascending q', and close with the same wave_sum; the library is built with
    -ffp-contract=off, so neither is contracted differently.  One fit on lds_row64 and one on the same rows followed by a row
    of 65 entries that no epoch visits (max_row is the data set's: that row alone moves every batch to the generic kernel):
    the same bits in P, w, the intercept, the sums and AdaGrad's state."""
    case = K.ROW_BY_NAME["lds_row64"]
    X, y = K.row_data(case.name)
    X65, y65 = K.with_one_more_row(X, 65), np.append(y, 0.25)
    assert K.row_kernel(case.k, case.F, int(X65.lengths().max())) == ("generic", 0) and case.kernel == "lds"
    perms = K.row_perms()
    ref = oracle_fit(X, y, case.k, solver, K.BATCH, perms)
    lds, n_lds = epochs_over_the_first_rows(X, y, case.k, solver, perms, X.n)
    gen, n_gen = epochs_over_the_first_rows(X65, y65, case.k, solver, perms, X.n)
    launches = K.row_launches(solver)
    assert (n_lds["ffm_row_lds"], n_lds["ffm_row_generic"], n_lds["ffm_row_coop"]) == (launches, 0, 0)
    assert (n_gen["ffm_row_lds"], n_gen["ffm_row_generic"], n_gen["ffm_row_coop"]) == (0, launches, 0)
    compare(lds, ref, solver, "lds")
    compare(gen, ref, solver, "generic")
    keys = [key for key in lds if key != "it"]
    assert_same_bits({key: lds[key] for key in keys}, {key: gen[key] for key in keys}, "%s: lds vs generic" % solver)


# ---------------------------------------------------------------- the column path
@pytest.mark.parametrize("solver,cap", [("sgd", 1.0), ("sgd", 16.0), ("adagrad", 1.0)])
@pytest.mark.parametrize("k", K.COL_KS)
@pytest.mark.parametrize("control", [False, True], ids=["counts", "control"])
def test_column_phase_at_exact_touch_counts(control, k, solver, cap):
    """features of exactly 1, 2, 63, 64, 65, 127, 128, 129 and 150 touches in every batch: the decay table and the pow branch of
    ffm_touch_factors, the ordinary unit at 128 touches, three segments at 129 (64, 64 and 1) and at 150.  The heavy kernels run
    in every batch that has such a feature -- all of SGD's, all of AdaGrad's but its first step of one sample -- and in none of
    the control set, whose largest count is 128."""
    X, y = K.col_data(control)
    ref = oracle_fit(X, y, k, solver, K.COL_BATCH, cap=cap)
    what = "column%s k %d %s cap %g" % (" control" if control else "", k, solver, cap)
    got, n = gpu_fit(X, to_gpu(to_oracle(X)), y, k, solver, K.COL_BATCH, cap=cap, timing=True)
    print("%s: %s" % (what, ", ".join("%s %d" % (f, n[f]) for f in COUNTED)))
    heavy = K.heavy_batches(X, K.COL_BATCH, solver)[0]
    assert heavy == (0 if control else 6)
    assert (n["heavy_partial"], n["heavy_apply"]) == (heavy, heavy), what
    assert n["row_phase"] == n[K.FAMILY[K.row_kernel(k, X.F, int(X.lengths().max()))[0]]] == len(K.fit_batches(X.n, K.COL_BATCH, solver))
    assert n["refresh"] == K.refresh_batches(X, K.COL_BATCH, solver)
    compare(got, ref, solver, what)


# ---------------------------------------------------------------- the refresh
@pytest.mark.parametrize("k", K.REFRESH_KS)
@pytest.mark.parametrize("regime", list(K.REFRESH))
def test_refresh_runs_where_a_batch_reads_its_features_four_times(regime, k):
    X, y = K.refresh_data(regime)
    ref = oracle_fit(X, y, k, "adagrad", K.COL_BATCH)
    what = "refresh %s k %d" % (regime, k)
    got, n = gpu_fit(X, to_gpu(to_oracle(X)), y, k, "adagrad", K.COL_BATCH, timing=True)
    print("%s: %s" % (what, ", ".join("%s %d" % (f, n[f]) for f in COUNTED)))
    want = K.refresh_batches(X, K.COL_BATCH, "adagrad")
    assert want == (6 if regime == "dense" else 0) and n["refresh"] == want, what
    assert n["row_phase"] == 7 and n["heavy_partial"] == n["heavy_apply"] == K.heavy_batches(X, K.COL_BATCH, "adagrad")[0]
    compare(got, ref, "adagrad", what)


# ---------------------------------------------------------------- decisionFunction
def model_for(X, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((X.F, X.d, k)) * 0.2, rng.standard_normal(X.d), -1.5


@pytest.mark.parametrize("F", K.PREDICT_FS)
@pytest.mark.parametrize("k", K.PREDICT_KS)
def test_ffm_decision_function_at_every_lane_width(k, F):
    """rows of 0, 1, 2, 63, 64, 65 and 130 entries (and one more where a column id is repeated), unsorted, 261 of them"""
    X = K.predict_data(F)
    Xo = to_oracle(X)
    P, w, b = model_for(X, k, 100 * k + F)
    want = O.ffm_decision_function(Xo, P, w, b)
    assert np.isfinite(want).all() and want[X.lengths() == 0].tolist() == [b] * int((X.lengths() == 0).sum())
    got = np.array(gpu_ffm("regression", k, True, True, P, w, b).decisionFunction(to_gpu(Xo)), dtype=np.float64)
    assert_close(got, want, 1e-10, 1e-12, "k %d F %d" % (k, F))


def test_ffm_decision_function_beyond_one_pass_of_the_grid():
    """more samples than n_cu * 32 workgroups have wavefronts: some wavefronts of k_ffm_predict take a second sample"""
    X = K.strided_data()
    Xo = to_oracle(X)
    P, w, b = model_for(X, 1, 5)
    want = O.ffm_decision_function(Xo, P, w, b)
    got = np.array(gpu_ffm("regression", 1, True, True, P, w, b).decisionFunction(to_gpu(Xo)), dtype=np.float64)
    assert got.shape == (K.STRIDED_N,)
    assert_close(got, want, 1e-10, 1e-12, "strided")


def test_ffm_decision_function_vs_brute_force_at_64_lanes():
    n, d, F, k = 40, 24, 3, 100
    Xo, Xd, field_of, _ = make_ffm_dataset(n, d, F, 2, 42, threshold=0.4)
    rng = np.random.default_rng(64)
    P, w, b = rng.standard_normal((F, d, k)) * 0.2, rng.standard_normal(d), -0.5
    got = np.array(gpu_ffm("regression", k, True, True, P, w, b).decisionFunction(to_gpu(Xo)), dtype=np.float64)
    assert K.lanes_for_k(k) == 64
    assert_close(got, O.ffm_decision_function(Xo, P, w, b), 1e-10, 1e-12, "oracle")
    assert_close(got, O.slow_ffm_decision_function(Xd, field_of, F, P, w, b), 1e-6, 1e-9, "brute force")
