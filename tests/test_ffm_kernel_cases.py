"""CPU: the conditions the inputs of tests/ffm_kernel_cases.py must meet so that tests/test_gpu_ffm_kernels.py runs the
field-aware mini-batch kernels (csrc/mb_ffm.hip) at every lane width under each of the three row kernels, on both sides of
every threshold of run_ffm, through the heavy path at exactly 128 and 129 touches and through k_ffm_refresh -- and that the
oracle's fit of every case is one worth comparing with.  No GPU: the restatement of the host's choice only, and the strings of
the sources it restates.  Run with -s to see the table."""
import os

import numpy as np
import pytest

import ffm_kernel_cases as K
import oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")
LS = (1, 2, 4, 8, 16, 32, 64)


def src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_source_still_has_the_choices_restated():
    ffm, common, plan_h, plan, pred = (src(f) for f in ("mb_ffm.hip", "common.h", "plan.h", "plan.hip", "predict.hip"))
    assert "constexpr int kWave = 64;" in common
    assert "int half = (k + 1) / 2, L = 1;" in common
    # run_ffm's own choices (row kernel, LDS bytes, counters, refresh, grids) are called, not read: tests/test_cpp_mb_ffm_route.py
    assert "getenv(" not in ffm
    assert "NFM_CHECK(M.Kp == 2 * M.L && M.Kp <= 128" in ffm
    assert 'TimedLaunch tl(ctx, "row_phase");' in ffm  # the family bench.py reads
    assert "constexpr int kFtab = 64;" in src("mb_dev.h") and "if (ci <= kFtab) {" in ffm
    assert "if (t1 - t0 <= kHeavyTouches)" in ffm
    assert "constexpr int kHeavyTouches = 128;" in plan_h and "constexpr int kHeavySegment = 64;" in plan_h
    assert "const bool heavy = c > kHeavyTouches;" in plan
    # (the boundaries are plan_route.h's plan_bounds, which tests/test_cpp_plan_route.py runs)
    assert "if (first_singleton && ns > 0) { pos = 1; B.bat_pos.push_back(1); }" in src("plan_route.h") and "= plan_bounds(ns, " in plan
    assert "int64_t blocks = (X.n + kWavesPerBlock - 1) / kWavesPerBlock;" in pred and "if (j1 < j2) {" in pred


def test_the_issue_s_byte_counts():
    """the figures of the table as the formula gives them"""
    want = {"lds_small": ("lds", 16320), "lds_big": ("lds", 83456), "lds_last": ("lds", 150016), "coop_first": ("coop", 38544),
            "coop_big_L32": ("coop", 82304), "coop_last_L64": ("coop", 152176), "generic_size_L64": ("generic", 0),
            "lds_row64": ("lds", 28800), "generic_row65": ("generic", 0), "coop_F64_m64_L1": ("coop", 67072),
            "generic_F65": ("generic", 0), "lds_big_k128": ("lds", 82624), "lds_L16": ("lds", 99520)}
    for name, (kernel, lds) in want.items():
        c = K.ROW_BY_NAME[name]
        assert (c.kernel, c.lds_bytes) == (kernel, lds), name
    assert K.per_wave_bytes(100, 4, 38) == 156288
    assert [K.lanes_for_k(k) for k in (1, 2, 3, 7, 13, 30, 33, 50, 64, 65, 100, 128)] == [1, 1, 2, 4, 8, 16, 32, 32, 32, 64, 64, 64]


def test_the_table_reaches_every_lane_width_under_every_kernel():
    got = {}
    for c in K.ROW_CASES:
        got.setdefault((c.kernel, K.lanes_for_k(c.k)), []).append(c)
        print("%-18s k %3d L %2d F %2d max_row %2d  %-7s %6d B%s" % (c.name, c.k, K.lanes_for_k(c.k), c.F, max(c.lengths), c.kernel, c.lds_bytes,
                                                                     "  (> 64 KiB)" if c.lds_bytes > K.LDS_DEFAULT else ""))
    assert set(got) == {(kernel, L) for kernel in ("lds", "coop", "generic") for L in LS}
    for kernel in ("lds", "coop"):  # two lane widths on either side of the 64 KiB a launch has without the attribute
        big = {L for (kn, L), cs in got.items() if kn == kernel and any(c.lds_bytes > K.LDS_DEFAULT for c in cs)}
        small = {L for (kn, L), cs in got.items() if kn == kernel and any(c.lds_bytes <= K.LDS_DEFAULT for c in cs)}
        assert len(big) >= 2 and len(small) >= 2, (kernel, big, small)
    assert all(0 < c.lds_bytes <= K.LDS_SHARE for c in K.ROW_CASES if c.kernel != "generic")
    # every L with a k that leaves padding lanes or a padding component
    assert {K.lanes_for_k(c.k) for c in K.ROW_CASES if c.k < 2 * K.lanes_for_k(c.k)} == set(LS)
    # R = 1 under all three kernels, the generic one with F > 64, with a row of 65 and with rows that fit by length only
    generic = [c for c in K.ROW_CASES if c.kernel == "generic"]
    assert any(c.F > 64 for c in generic) and any(max(c.lengths) > 64 and c.F <= 64 for c in generic)
    assert any(max(c.lengths) <= 64 and c.F <= 64 for c in generic)
    for c in K.ROW_CASES:
        assert c.lengths[0] == max(c.lengths) and {0, 1} <= set(c.lengths) and c.F <= K.D_TRAIN and max(c.lengths) <= K.D_TRAIN - K.N_HUBS
    assert set(K.FLAG_CASES) <= set(K.ROW_BY_NAME) and {K.ROW_BY_NAME[n].kernel for n in K.FLAG_CASES} == {"lds", "coop", "generic"}
    assert len(set(K.FLAGS)) == 4


def test_each_threshold_pair_straddles_its_threshold():
    a, b = (K.ROW_BY_NAME[n] for n in K.THRESHOLD_PAIRS[0])  # four samples per workgroup / one
    assert (a.k, a.F) == (b.k, b.F) and max(b.lengths) == max(a.lengths) + 1
    assert 4 * K.per_wave_bytes(a.k, a.F, max(a.lengths)) <= K.LDS_SHARE < 4 * K.per_wave_bytes(b.k, b.F, max(b.lengths))
    assert (a.kernel, b.kernel) == ("lds", "coop")
    a, b = (K.ROW_BY_NAME[n] for n in K.THRESHOLD_PAIRS[1])  # the LDS share itself
    assert (a.k, a.F) == (b.k, b.F) and max(b.lengths) == max(a.lengths) + 1 <= 64
    assert K.per_wave_bytes(a.k, a.F, max(a.lengths)) <= K.LDS_SHARE < K.per_wave_bytes(b.k, b.F, max(b.lengths))
    assert (a.kernel, b.kernel) == ("coop", "generic")
    a, b = (K.ROW_BY_NAME[n] for n in K.THRESHOLD_PAIRS[2])  # a row of 64 entries / of 65
    assert (a.k, a.F) == (b.k, b.F) and (max(a.lengths), max(b.lengths)) == (64, 65)
    assert K.row_kernel(b.k, b.F, 64) == (a.kernel, a.lds_bytes) and a.kernel != "generic" and b.kernel == "generic"
    a, b = (K.ROW_BY_NAME[n] for n in K.THRESHOLD_PAIRS[3])  # 64 fields / 65
    assert a.k == b.k and (a.F, b.F) == (64, 65) and max(a.lengths) == 64
    assert K.row_kernel(b.k, 64, max(b.lengths))[0] != "generic" and a.kernel != "generic" and b.kernel == "generic"
    # the 64 KiB of a launch without the attribute: the same kernel on both sides
    a, b = K.ROW_BY_NAME["lds_small"], K.ROW_BY_NAME["lds_big"]
    assert a.kernel == b.kernel == "lds" and a.lds_bytes <= K.LDS_DEFAULT < b.lds_bytes
    a, b = K.ROW_BY_NAME["coop_first"], K.ROW_BY_NAME["coop_big_L32"]
    assert a.kernel == b.kernel == "coop" and a.lds_bytes <= K.LDS_DEFAULT < b.lds_bytes


@pytest.mark.parametrize("case", K.ROW_CASES, ids=lambda c: c.name)
def test_row_data_is_as_stated(case):
    X, y = K.row_data(case.name)
    assert (X.n, X.d, X.F, len(y)) == (K.N_TRAIN, K.D_TRAIN, case.F, K.N_TRAIN)
    assert X.lengths().tolist() == [case.lengths[i % len(case.lengths)] for i in range(X.n)]
    assert int(X.lengths()[0]) == int(X.lengths().max()) == max(case.lengths)
    field_of = np.full(X.d, -1)
    unsorted = 0
    for i in range(X.n):
        row = X.row(i)
        assert len(np.unique(row)) == len(row) and (len(row) == 0 or (row.min() >= 0 and row.max() < X.d))
        assert int((row < K.N_HUBS).sum()) == (2 if len(row) >= 2 else 0)
        f = X.fields[X.indptr[i]:X.indptr[i + 1]]
        assert ((field_of[row] == -1) | (field_of[row] == f)).all()  # the field is the feature's
        field_of[row] = f
        if i % 2 == 0 and len(row) >= 2:
            assert np.all(np.diff(row) > 0)
        elif len(row) >= 2:
            assert not np.all(np.diff(row) > 0)
            unsorted += 1
    assert unsorted >= X.n // len(case.lengths)
    assert set(field_of[field_of >= 0].tolist()) == set(range(case.F))  # every field present
    assert np.abs(X.data).max() < 1.0
    perms = K.row_perms()
    assert perms.shape == (K.EPOCHS, X.n) and all(sorted(p.tolist()) == list(range(X.n)) for p in perms) and perms[0][0] == 0
    assert [len(ids) for ids, _ in K.fit_batches(X.n, K.BATCH, "sgd", perms)] == [77, 77, 77, 69] * 2
    assert [len(ids) for ids, _ in K.fit_batches(X.n, K.BATCH, "adagrad", perms)] == [1, 77, 77, 77, 68, 77, 77, 77, 69]
    assert [s for _, s in K.fit_batches(X.n, K.BATCH, "adagrad", perms)] == [True] + [False] * 8
    assert (K.row_launches("sgd"), K.row_launches("adagrad")) == (8, 9)
    # the longest row in a full batch of both solvers' first epoch besides AdaGrad's stored step: the widest sample is run
    # by the kernel under test with the state's parameters as well
    longest = set(np.flatnonzero(X.lengths() == max(case.lengths)).tolist())
    for solver in ("sgd", "adagrad"):
        assert all(longest & set(ids.tolist()) for ids, stored in K.fit_batches(X.n, K.BATCH, solver, perms) if not stored)


def to_oracle(X):
    return O.Dataset(X.indptr, X.indices, X.data, X.n, X.d, X.fields, X.F)


def oracle_fit(X, y, k, solver, batch, perms=None, fit_linear=True, fit_intercept=True, cap=1.0, n_fit=None):
    """EPOCHS epochs of the mini-batch rule on the CPU (oracle/nimfm_mb.c) over the first n_fit positions: everything the GPU tests compare"""
    Xo = to_oracle(X)
    P0, w0, b0 = K.start(X.d, X.F, k, fit_linear)
    P, w, b, it = P0.copy(), w0.copy(), b0, 1
    n_fit = X.n if n_fit is None else n_fit
    st = O.AdaState(X.F, X.d, k, X.d)
    viol, loss = [], []
    for e in range(K.EPOCHS):
        perm = None if perms is None else perms[e]
        if solver == "sgd":
            cfg = O.sgd_cfg(eta0=K.SGD_ETA0, fit_linear=fit_linear, fit_intercept=fit_intercept)
            b, it, ls, vs = O.ffm_sgd_epoch_mb(Xo, y, P, w, b, cfg, batch, perm=perm, end=n_fit, it=it, touch_cap=cap)
        else:
            cfg = O.adagrad_cfg(eta0=K.ADA_ETA0, fit_linear=fit_linear, fit_intercept=fit_intercept)
            b, it, ls, vs = O.ffm_adagrad_epoch_mb(Xo, y, P, w, b, cfg, batch, st, perm=perm, end=n_fit, it=it)
        viol.append(vs)
        loss.append(ls / n_fit)
    out = {"P0": P0, "P": P, "w": w, "b": b, "it": it, "viol": np.array(viol), "loss": np.array(loss)}
    if solver == "adagrad":
        out["b"] = O.ffm_adagrad_finalize(P, w, b, cfg, it, st)
        out.update(g_sum=st.gsum_P, g_norm=st.gnorm_P)
    return out


def assert_usable(ref, what, touched=None):
    """finite, the second epoch's loss below the first's, and at least 90 % of P's entries moved (of the touched features'
    where the data set leaves most of a large table alone)"""
    assert all(np.isfinite(ref[key]).all() for key in ("P", "w", "b", "viol", "loss")), what
    assert ref["loss"][1] < ref["loss"][0], (what, ref["loss"])
    P, P0 = (ref["P"], ref["P0"]) if touched is None else (ref["P"][:, touched], ref["P0"][:, touched])
    assert (P != P0).mean() >= 0.9, (what, (P != P0).mean())
    print("%s: loss %.4f -> %.4f, P nonzero %.3f" % (what, ref["loss"][0], ref["loss"][1], (ref["P"] != 0.0).mean()))


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
@pytest.mark.parametrize("case", K.ROW_CASES, ids=lambda c: c.name)
def test_the_oracle_s_fit_of_every_row_case_is_usable(case, solver):
    X, y = K.row_data(case.name)
    assert_usable(oracle_fit(X, y, case.k, solver, K.BATCH, K.row_perms()), "%s %s" % (case.name, solver))


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
@pytest.mark.parametrize("flags", K.FLAGS, ids=lambda f: "lin%d_b%d" % f)
@pytest.mark.parametrize("name", K.FLAG_CASES)
def test_the_oracle_s_fit_with_every_flag_is_usable(name, flags, solver):
    case = K.ROW_BY_NAME[name]
    X, y = K.row_data(name)
    ref = oracle_fit(X, y, case.k, solver, K.BATCH, K.row_perms(), *flags)
    assert_usable(ref, "%s %s %s" % (name, flags, solver))
    P0, w0, b0 = K.start(X.d, X.F, case.k, flags[0])
    assert flags[0] or (ref["w"] == 0.0).all()
    assert flags[1] or ref["b"] == b0


# ---------------------------------------------------------------- the column path
@pytest.mark.parametrize("control", [False, True], ids=["counts", "control"])
def test_column_data_has_exactly_the_stated_counts(control):
    X, y = K.col_data(control)
    counts = K.CONTROL_COUNTS if control else K.COUNTS
    assert K.COUNTS == (1, 2, 63, 64, 65, 127, 128, 129, 150) and max(K.CONTROL_COUNTS) == K.kHeavyTouches
    assert (X.n, X.d, X.F, K.COL_BATCH) == (450, 400, 3, 150)
    cuts = [ids for ids, _ in K.fit_batches(X.n, K.COL_BATCH, "sgd")]
    assert [len(ids) for ids in cuts] == [150] * 6
    for ids in cuts:
        c = K.batch_counts(X, ids)
        assert tuple(c[:len(counts)].tolist()) == counts
        assert c[len(counts):].sum() == 3 * len(ids) and c[len(counts):].max() <= 63  # the others: on the table's side of kFtab
    assert X.lengths().min() >= 3 and int(X.lengths()[0]) == int(X.lengths().max()) == 3 + len(counts)
    for i in range(X.n):
        row = X.row(i)
        assert len(np.unique(row)) == len(row)
        assert (np.all(np.diff(row) > 0)) == (i % 2 == 0)
    # AdaGrad's first epoch: 1, 150, 150, 149 -- the full windows keep their counts, the last one loses one touch per feature
    ada = K.fit_batches(X.n, K.COL_BATCH, "adagrad")
    assert [len(ids) for ids, _ in ada] == [1, 150, 150, 149, 150, 150, 150]
    assert [tuple(K.batch_counts(X, ids)[:len(counts)].tolist()) for ids, _ in ada[1:3]] == [counts] * 2
    assert tuple(K.batch_counts(X, ada[3][0])[:len(counts)].tolist()) == tuple(c - 1 for c in counts)
    for solver in ("sgd", "adagrad"):
        n_heavy, segs = K.heavy_batches(X, K.COL_BATCH, solver)
        assert (n_heavy, segs) == ((0, 0) if control else (6, 3)), solver  # 150 touches: segments of 64, 64 and 22; 129: 64, 64 and 1
    assert {K.lanes_for_k(k) for k in K.COL_KS} == {1, 8, 32, 64} and all(k < 2 * K.lanes_for_k(k) for k in K.COL_KS)
    assert K.COL_CAPS == (1.0, 16.0) and 65 > K.kFtab and 65 / 16.0 > 1.0 and 64 <= K.kFtab


@pytest.mark.parametrize("k", K.COL_KS)
@pytest.mark.parametrize("control", [False, True], ids=["counts", "control"])
def test_the_oracle_s_fit_of_the_column_data_is_usable(control, k):
    X, y = K.col_data(control)
    for solver, cap in (("sgd", 1.0), ("sgd", 16.0), ("adagrad", 1.0)):
        assert_usable(oracle_fit(X, y, k, solver, K.COL_BATCH, cap=cap), "column k %d %s cap %g" % (k, solver, cap))


# ---------------------------------------------------------------- the refresh
@pytest.mark.parametrize("regime", list(K.REFRESH))
def test_refresh_regimes_are_what_they_claim(regime):
    X, y = K.refresh_data(regime)
    assert (X.n, X.d, X.F) == (K.COL_N, K.REFRESH[regime], K.COL_F)
    for ids, stored in K.fit_batches(X.n, K.COL_BATCH, "adagrad"):
        c = K.batch_counts(X, ids)
        if regime == "dense":
            assert stored or c.sum() >= 4 * np.count_nonzero(c)
        else:
            assert c.sum() < 4 * np.count_nonzero(c)
    assert K.refresh_batches(X, K.COL_BATCH, "adagrad") == (6 if regime == "dense" else 0)
    assert K.refresh_batches(X, K.COL_BATCH, "sgd") == 0
    assert {K.lanes_for_k(k) for k in K.REFRESH_KS} == {1, 32, 64}
    touched = np.unique(X.indices)
    for k in K.REFRESH_KS:
        assert_usable(oracle_fit(X, y, k, "adagrad", K.COL_BATCH), "refresh %s k %d" % (regime, k), touched)


# ---------------------------------------------------------------- decisionFunction
@pytest.mark.parametrize("F", K.PREDICT_FS)
def test_predict_data(F):
    X = K.predict_data(F)
    assert (X.n, X.d, X.F) == (261, 200, F) and X.n % 4 == 1
    dup = 0
    for i in range(X.n):
        row, want = X.row(i), K.PREDICT_LENGTHS[i % len(K.PREDICT_LENGTHS)]
        if i % 5 == 2 and want >= 2:
            assert len(row) == want + 1 and row[-1] == row[0] and len(np.unique(row)) == want
            dup += 1
        else:
            assert len(row) == want and len(np.unique(row)) == want
    assert dup >= 20 and set(K.PREDICT_LENGTHS) == {0, 1, 2, 63, 64, 65, 130}
    assert {K.lanes_for_k(k) for k in K.PREDICT_KS} == set(LS) and K.PREDICT_FS == (1, 3, 65)
    seen = set(X.fields.tolist())
    assert seen <= set(range(F)) and len(seen) == F
    S = K.strided_data()
    assert S.n > 256 * 32 * 4 and set(S.lengths().tolist()) == {0, 1, 2, 3} and S.F == 2
    assert all(len(np.unique(S.row(i))) == len(S.row(i)) for i in range(0, S.n, 97))
