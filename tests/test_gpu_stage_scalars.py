"""-m gpu: the staged scalar streams of the headline's kernels (k_stage_dl / NFM_STAGE_DL, k_stage_w / NFM_STAGE_W) against the
gathers they stand in for (bit for bit) and against the mini-batch oracle (oracle/nimfm_mb.c).

k_stage_dl puts a batch's dL in column-phase touch order for k_col_long's compact variant; k_stage_w puts the linear weights of
a batch's entries in sample order for the held-entries row phase of SGD.  Every case trains twice, both parts forced on
(NFM_STAGE_DL=1 NFM_STAGE_W=1) and both forced off (0 / 0), with NFM_COL_LONG=1 NFM_COL_GRID=3 so that lane groups walk
several features and lists longer than one block of 32 touches occur at d = 512; the library counts the staging launches it
enqueues (nfm_ctx_timing_get "stage_dl" / "stage_w"), so every case also says which parts it expects to have run."""
import numpy as np
import pytest

import nimfm_amd as nf
import oracle as O
from common import assert_close, make_perms, random_csr
from gpu_common import _env, gpu_fm, ragged_csr, to_gpu
from test_gpu_col_long import assert_same_bits, oracle_train, start, train

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
N, D, K, B = 3000, 512, 64, 1024  # batches of 1024, 1024 and 952 samples: the last one short and ragged against the buffers


def staged(ctx):
    return np.array([ctx.timing_get("stage_dl")[0], ctx.timing_get("stage_w")[0]])


def both_ways(ctx, fn, expect_dl, expect_w, **env):
    """fn() with both parts forced on, then forced off; the two results, bitwise equal, and the launches counted"""
    base = dict(NFM_COL_LONG=1, NFM_COL_GRID=3)
    base.update(env)
    res = []
    for on in (1, 0):
        c0 = staged(ctx)
        with _env(NFM_STAGE_DL=on, NFM_STAGE_W=on, **base):
            res.append(fn())
        c = staged(ctx) - c0
        if on:
            assert (c[0] > 0) == expect_dl and (c[1] > 0) == expect_w, "staging launches (dL, w) = %s" % c
        else:
            assert (c == 0).all(), "staging launches with both knobs 0: %s" % c
    assert_same_bits(res[0], res[1], "staged vs gathered")
    return res[0]


def check(solver, Xo, y, k, P0, w0, batch, expect_dl=True, expect_w=True, perms=None, fit_linear=True, gpu_kw=None, orc_kw=None, **env):
    Xg = to_gpu(Xo)
    gpu_kw, orc_kw = gpu_kw or {}, orc_kw or {}
    new = both_ways(Xg.ctx, lambda: train(solver, Xg, y, k, P0, w0, batch, perms, fit_linear, 1, **gpu_kw), expect_dl, expect_w, **env)
    ref = oracle_train(solver, Xo, y, k, P0, w0, batch, perms, fit_linear, 1, **orc_kw)
    assert abs(new["b"][0] - ref["b"]) < 1e-11
    assert_close(new["w"], ref["w"], RTOL, ATOL, "w")
    assert_close(new["P"], ref["P"], RTOL, ATOL, "P")


@pytest.fixture(scope="module")
def full_rows():
    Xo = random_csr(N, D, 64, seed=21)
    y = np.random.default_rng(22).standard_normal(N)
    return (Xo, y) + start(D, K, 23)


def test_full_rows(full_rows):
    Xo, y, P0, w0 = full_rows
    check("sgd", Xo, y, K, P0, w0, B)


def test_ragged_rows_with_empty_samples():
    """rows of 0 ... 64 entries, every seventh empty, every other one stored unsorted"""
    Xo = ragged_csr(N, D, seed=24, max_m=64, empty_every=7)
    lens = np.diff(Xo.indptr)
    assert lens.min() == 0 and lens.max() == 64
    y = np.random.default_rng(25).standard_normal(N)
    P0, w0 = start(D, K, 26)
    check("sgd", Xo, y, K, P0, w0, B)


def test_rows_stored_unsorted():
    Xo = random_csr(N, D, 24, seed=27, sorted_idx=False)
    assert (np.diff(Xo.indices.reshape(N, 24), axis=1) < 0).any()
    y = np.random.default_rng(28).standard_normal(N)
    P0, w0 = start(D, K, 29)
    check("sgd", Xo, y, K, P0, w0, B)


def test_host_permutation(full_rows):
    Xo, y, P0, w0 = full_rows
    check("sgd", Xo, y, K, P0, w0, B, perms=make_perms(N, 2))


def by_hand(Xg, y, k, P0, w0, batch, calls, seed=None, solver="sgd"):
    """epoch calls over the ranges of `calls` on one optimizer; seed: the order is drawn on the device"""
    from nimfm_amd import _capi as capi
    fm = gpu_fm("regression", 2, k, "explicit", True, True, P0, w0, 0.0)
    opt = (nf.newSGD if solver == "sgd" else nf.newAdaGrad)(maxIter=1, verbose=0, tol=0, shuffle=seed is not None, mode="minibatch", batch=batch,
                                                             deviceShuffle=seed is not None)
    Xg.set_targets(y)
    opt._handle(fm, Xg.ctx, "minibatch")
    if seed is not None:
        capi.check(capi.lib().nfm_opt_set_shuffle(opt._h, seed))
    hist, perms = [], []
    for lo, hi in calls:
        hist.append(opt._epoch(Xg, None, lo, hi))
        opt.it += hi - lo
        if seed is not None:
            perms.append(opt.last_permutation(hi - lo))
    opt._finalize_into(fm)
    out = {"P": np.array(fm.P), "w": np.array(fm.w), "b": np.array([fm.intercept]), "loss": np.array([h[0] for h in hist]),
           "viol": np.array([h[1] for h in hist])}
    if perms:
        out["perms"] = np.stack(perms).astype(np.float64)  # (compared by bits like the rest)
    return out


def test_device_drawn_order(full_rows):
    Xo, y, P0, w0 = full_rows
    Xg = to_gpu(Xo)
    new = both_ways(Xg.ctx, lambda: by_hand(Xg, y, K, P0, w0, B, [(0, N)] * 2, seed=7), True, True)
    P, w, b, it = P0.copy(), w0.copy(), 0.0, 1
    for e in range(2):
        b, it, ls, vs = O.fm_sgd_epoch_mb(Xo, y, 2, P, w, b, O.sgd_cfg(), B, perm=new["perms"][e].astype(np.int64), it=it)
        assert_close([ls, vs], [new["loss"][e], new["viol"][e]], 1e-9, 0, "loss / viol of epoch %d" % e)
    assert abs(new["b"][0] - b) < 1e-11
    assert_close(new["w"], w, RTOL, ATOL, "w")
    assert_close(new["P"], P, RTOL, ATOL, "P")


def test_sub_range_calls(full_rows):
    """three epoch calls over consecutive ranges (the nCalls callbacks): every call's first batch stages its weights before
    its first row phase, from the w the previous call left"""
    Xo, y, P0, w0 = full_rows
    Xg = to_gpu(Xo)
    calls = [(0, 700), (700, 2950), (2950, N)]
    new = both_ways(Xg.ctx, lambda: by_hand(Xg, y, K, P0, w0, B, calls), True, True)
    P, w, b, it = P0.copy(), w0.copy(), 0.0, 1
    for c, (lo, hi) in enumerate(calls):
        b, it, ls, vs = O.fm_sgd_epoch_mb(Xo, y, 2, P, w, b, O.sgd_cfg(), B, begin=lo, end=hi, it=it)
        assert_close([ls, vs], [new["loss"][c], new["viol"][c]], 1e-9, 1e-12, "loss / viol of [%d, %d)" % (lo, hi))
    assert abs(new["b"][0] - b) < 1e-11
    assert_close(new["w"], w, RTOL, ATOL, "w")
    assert_close(new["P"], P, RTOL, ATOL, "P")


def test_graph_replay(full_rows):
    """12 batches of 256: the first epoch call captures the launches (staging kernels included) as a graph, the second
    replays it"""
    Xo, y, P0, w0 = full_rows
    check("sgd", Xo, y, K, P0, w0, 256)


def test_several_slices_and_their_boundaries():
    """d = 600000: k_stage_w works in three slices of 200000 features; the first and the last feature of every slice occur, in
    both batches, in rows that mix the slices.  (k = 16, and NFM_SINGLES=0: at this touch rate the row phase would otherwise
    update the single-touch features itself, in the register-resident mode that is not staged.)"""
    n, d, m, k = 2048, 600000, 8, 16
    Xo = random_csr(n, d, m, seed=31, sorted_idx=False)
    edges = np.array([0, 199999, 200000, 399999, 400000, 599999])
    rng = np.random.default_rng(32)
    for i in (0, 1, 500, 1023, 1024, 1500, 2047):
        row = np.concatenate([edges, rng.choice(np.arange(1, 199999), 2, replace=False)])
        Xo.indices[i * m:(i + 1) * m] = rng.permutation(row)
    y = rng.standard_normal(n)
    P0, w0 = start(d, k, 33)
    check("sgd", Xo, y, k, P0, w0, B, NFM_SINGLES=0)


def test_without_linear_term(full_rows):
    Xo, y, P0, w0 = full_rows
    check("sgd", Xo, y, K, P0, w0, B, expect_w=False, fit_linear=False)


def test_adagrad_stages_dl_only(full_rows):
    Xo, y, P0, w0 = full_rows
    check("adagrad", Xo, y, K, P0, w0, B, expect_w=False)


def test_pow_schedule_stages_nothing(full_rows):
    """invscaling at power 0.5: k_col_long takes the records (its non-compact variant), the batch is left as it was"""
    Xo, y, P0, w0 = full_rows
    kw = {"scheduling": "invscaling", "power": 0.5}
    check("sgd", Xo, y, K, P0, w0, B, expect_dl=False, expect_w=False, gpu_kw=kw, orc_kw=kw)


def test_data_parallel_exchange_after_every_batch(full_rows):
    """world 1 through RCCL, sync_period 1: every batch is a graph segment of its own and w changes outside the capture, so
    k_stage_w must sit at the head of the batch behind the exchange.  Staged segments against staged direct launches
    (NFM_DP_GRAPH=0) and against the gathers."""
    from nimfm_amd import dp
    Xo, y, P0, w0 = full_rows
    ctx = nf.default_context()
    grp = dp.Group.rccl(ctx, dp.Group.unique_id(), 0, 1)
    try:
        X = nf.CSRDataset(Xo.data, Xo.indices, Xo.indptr, N, D, ctx=ctx)

        def fit():
            fm = gpu_fm("regression", 2, K, "explicit", True, True, P0, w0, 0.0)
            opt = nf.newSGD(maxIter=2, verbose=0, tol=0, shuffle=False, mode="minibatch", batch=256)
            opt.setDataParallel(grp, 1, True)
            opt.fit(X, y, fm)
            return {"P": np.array(fm.P), "w": np.array(fm.w), "b": np.array([fm.intercept]),
                    "viol": np.array([h[0] for h in opt.history]), "loss": np.array([h[1] for h in opt.history])}

        seg = both_ways(ctx, fit, True, True, NFM_DP_GRAPH=1)
        with _env(NFM_COL_LONG=1, NFM_COL_GRID=3, NFM_STAGE_DL=1, NFM_STAGE_W=1, NFM_DP_GRAPH=0):
            direct = fit()
        assert_same_bits(seg, direct, "graph segments vs direct launches")
        assert np.isfinite(seg["P"]).all() and not np.array_equal(seg["P"], P0)
    finally:
        grp.close()
