"""-m gpu: the column phase for long touch lists (k_col_long, NFM_COL_LONG) against the kernels it stands in for
(bit for bit) and against the mini-batch oracle (oracle/nimfm_mb.c).

NFM_COL_LONG=1 takes the new kernel for every batch of a one-order degree-2 model, NFM_COL_LONG=0 never; NFM_COL_GRID=n
gives the column phase n feature workgroups that stride over the batch's features, so that a lane group walks several
features in a row (the headline's situation) on shapes of a few hundred features.  Both runs of a comparison get the same
grid: the viol sum depends on which workgroup adds which feature."""
import numpy as np
import pytest

import nimfm_amd as nf
import oracle as O
from common import assert_close, make_perms, random_csr
from gpu_common import _env, gpu_fm, to_gpu

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
EPOCHS = 2


def exact_lists_csr(d, m, batches, counts, seed):
    """CSR of sum(batches) rows with m distinct features each.  In every batch (consecutive rows) one feature is touched
    exactly c times for every c of counts, and every other feature that occurs is touched twice (one of them three times
    where the number of touches left over is odd)."""
    rng = np.random.default_rng(seed)
    idx, val = [], []
    for B in batches:
        left = B * m - sum(counts)
        assert left >= 0 and max(counts) <= B
        lens = sorted(list(counts) + [2] * (left // 2 - (left % 2)) + ([3] if left % 2 else []), reverse=True)
        assert sum(lens) == B * m and len(lens) <= d
        feats = rng.permutation(d)[:len(lens)]
        rows = [[] for _ in range(B)]
        for f, c in zip(feats, lens):  # the c emptiest rows: distinct features per row, every row ends with m entries
            for r in sorted(range(B), key=lambda r: (len(rows[r]), r))[:c]:
                rows[r].append(f)
        assert all(len(r) == m for r in rows)
        for r in rows:
            idx.append(np.sort(np.array(r, dtype=np.int64)))
            val.append(rng.uniform(-1, 1, m))
    n = sum(batches)
    return O.Dataset(np.arange(n + 1, dtype=np.int64) * m, np.concatenate(idx), np.concatenate(val), n, d)


def train(solver, Xg, y, k, P0, w0, batch, perms=None, fit_linear=True, it0=1, **kw):
    """EPOCHS epochs through the C ABI; everything a caller can read back, as float64 arrays"""
    fm = gpu_fm("regression", 2, k, "explicit", fit_linear, True, P0, w0, 0.0)
    if solver == "sgd":
        opt = nf.newSGD(maxIter=EPOCHS, verbose=0, tol=0, shuffle=perms is not None, mode="minibatch", batch=batch, **kw)
    else:
        opt = nf.newAdaGrad(maxIter=EPOCHS, verbose=0, tol=0, shuffle=perms is not None, mode="minibatch", batch=batch, **kw)
    opt.it = it0
    if perms is None:
        opt.fit(Xg, y, fm)
    else:
        opt.fit(Xg, y, fm, perms=perms)
    out = {"P": np.array(fm.P), "w": np.array(fm.w), "b": np.array([fm.intercept]),
           "viol": np.array([h[0] for h in opt.history]), "loss": np.array([h[1] for h in opt.history])}
    if solver == "adagrad":
        gs, gn, gsw, gnw, gsb, gnb = opt.get_state(fm)
        out.update(g_sum=np.array(gs), g_norm=np.array(gn), g_sum_w=np.array(gsw), g_norm_w=np.array(gnw))
    return out


def oracle_train(solver, Xo, y, k, P0, w0, batch, perms=None, fit_linear=True, it0=1, touch_cap=1.0, ada_cross=0.0, **cfg_kw):
    P, w, b, it = P0.copy(), w0.copy(), 0.0, it0
    if solver == "sgd":
        cfg = O.sgd_cfg(fit_linear=fit_linear, **cfg_kw)
        for e in range(EPOCHS):
            b, it, _, _ = O.fm_sgd_epoch_mb(Xo, y, 2, P, w, b, cfg, batch, perm=None if perms is None else perms[e], it=it,
                                            touch_cap=touch_cap)
        return {"P": P, "w": w, "b": b}
    cfg = O.adagrad_cfg(fit_linear=fit_linear)
    st = O.AdaState(1, Xo.d, k, Xo.d)
    for e in range(EPOCHS):
        b, it, _, _ = O.fm_adagrad_epoch_mb(Xo, y, 2, P, w, b, cfg, batch, st, perm=None if perms is None else perms[e], it=it,
                                            ada_cross=ada_cross)
    b = O.fm_adagrad_finalize(2, P, w, b, cfg, it, st)
    return {"P": P, "w": w, "b": b, "g_sum": st.gsum_P, "g_norm": st.gnorm_P}


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        same = a[key].view(np.uint64) == b[key].view(np.uint64)
        assert same.all(), "%s: %s differs in %d of %d values" % (what, key, (~same).sum(), same.size)


def check(solver, Xo, y, k, P0, w0, batch, grid, perms=None, fit_linear=True, it0=1, gpu_kw=None, orc_kw=None):
    Xg = to_gpu(Xo)
    gpu_kw, orc_kw = gpu_kw or {}, orc_kw or {}
    with _env(NFM_COL_LONG=1, NFM_COL_GRID=grid):
        new = train(solver, Xg, y, k, P0, w0, batch, perms, fit_linear, it0, **gpu_kw)
    with _env(NFM_COL_LONG=0, NFM_COL_GRID=grid):
        old = train(solver, Xg, y, k, P0, w0, batch, perms, fit_linear, it0, **gpu_kw)
    assert_same_bits(new, old, "NFM_COL_LONG=1 vs 0")
    ref = oracle_train(solver, Xo, y, k, P0, w0, batch, perms, fit_linear, it0, **orc_kw)
    assert abs(new["b"][0] - ref["b"]) < 1e-11
    assert_close(new["w"], ref["w"], RTOL, ATOL, "w")
    assert_close(new["P"], ref["P"], RTOL, ATOL, "P")
    if solver == "adagrad":
        assert_close(new["g_sum"], ref["g_sum"], RTOL, ATOL, "g_sum")
        assert_close(new["g_norm"], ref["g_norm"], RTOL, 1e-20, "g_norm")
    if not fit_linear:
        assert (new["w"] == 0).all()


def start(d, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((1, k, d)) * (0.1 / np.sqrt(k)), np.zeros(d)


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
@pytest.mark.parametrize("k", [64, 16])
def test_exact_list_lengths(k, solver):
    """Lists of 3, D, D + 1 (D = 4 and 8: both ring depths that are built), L - 1, L, L + 1 (one block, its edge, two blocks),
    2L + 3 (three blocks), 128 (the longest the walk takes) and 129 touches (left to the heavy path) among lists of two, in
    two batches, the second shorter.  One feature workgroup: the features go round its lane groups by descending count, so
    each group walks from a long list into short ones, the first group from the skipped heavy feature into a long one.
    (AdaGrad's first epoch opens with a batch of one sample, which moves that epoch's batches by a row and its counts by
    at most one; its second epoch has the batches as constructed.)"""
    L = k // 2
    counts = sorted({3, 4, 5, 8, 9, L - 1, L, L + 1, 2 * L + 3, 128, 129})
    d, m, batches = 2048, 8, (256, 200)
    Xo = exact_lists_csr(d, m, batches, counts, seed=k)
    for lo, hi in ((0, batches[0]), (batches[0], sum(batches))):  # the construction is what the test is about
        got = np.bincount(Xo.indices[Xo.indptr[lo]:Xo.indptr[hi]], minlength=d)
        assert set(counts) <= set(got.tolist()) <= set(counts) | {0, 2}
    y = np.random.default_rng(k + 1).standard_normal(Xo.n)
    P0, w0 = start(d, k, 3)
    check(solver, Xo, y, k, P0, w0, batches[0], grid=1)


@pytest.fixture(scope="module")
def random_shape():
    n, d, m, k = 8192 + 100, 2048, 8, 64
    Xo = random_csr(n, d, m, seed=11)
    y = np.random.default_rng(12).standard_normal(n)
    P0, w0 = start(d, k, 13)
    return Xo, y, k, P0, w0


B = 4096  # 16 touches per feature and batch


@pytest.mark.parametrize("cap", [1.0, 8.0, 32.0])
def test_random_shape_sgd_touch_cap(random_shape, cap):
    Xo, y, k, P0, w0 = random_shape
    check("sgd", Xo, y, k, P0, w0, B, grid=2, gpu_kw={"touchCap": cap}, orc_kw={"touch_cap": cap})


@pytest.mark.parametrize("cross", [0.0, 0.1])
def test_random_shape_adagrad_cross(random_shape, cross):
    Xo, y, k, P0, w0 = random_shape
    check("adagrad", Xo, y, k, P0, w0, B, grid=2, gpu_kw={"adaCross": cross}, orc_kw={"ada_cross": cross})


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
def test_random_shape_without_linear_term(random_shape, solver):
    """(fitLinear on is every other case) -- and the grid run_batches chooses by itself: one feature per lane group"""
    Xo, y, k, P0, w0 = random_shape
    check(solver, Xo, y, k, P0, w0, B, grid=None, fit_linear=False)


@pytest.mark.parametrize("sched", ["constant", "optimal", "invscaling", "pegasos"])
def test_random_shape_schedules(random_shape, sched):
    Xo, y, k, P0, w0 = random_shape
    kw = {"scheduling": sched, "power": 0.5}
    it0 = 1
    if sched == "pegasos":  # eta = 1 / (reg * it) needs reg ~ 1 to stay finite, and 1 - eta * reg is 0 at it == 1
        kw.update(alpha0=0.5, alpha=0.5, beta=0.5)
        it0 = 20
    check("sgd", Xo, y, k, P0, w0, B, grid=2, it0=it0, gpu_kw=kw, orc_kw=kw)


def test_random_shape_with_permutation(random_shape):
    Xo, y, k, P0, w0 = random_shape
    check("sgd", Xo, y, k, P0, w0, B, grid=3, perms=make_perms(Xo.n, EPOCHS))


COL_COUNTERS = ["route_col_" + c for c in ("long", "long_compact", "phase", "strided", "sparse", "tu1", "tu4")]


def col_counts(ctx):
    """(batches that took k_col_long, either variant; batches in all) so far: the driver counts one route_col_* per batch it
    enqueues (nfm_ctx_timing_get)"""
    c = [ctx.timing_get(name)[0] for name in COL_COUNTERS]
    return np.array([c[0] + c[1], sum(c)])


@pytest.mark.parametrize("batch", [256, 4096])
def test_selection_by_itself_keeps_the_bits(random_shape, batch):
    """NFM_COL_LONG unset: two touches per feature (below the threshold) and 16 (above it), on a strided grid, both train to
    the bits of NFM_COL_LONG=0 -- and the route says so: no batch on k_col_long at two touches, some at sixteen, none under
    NFM_COL_LONG=0, every one under NFM_COL_LONG=1"""
    Xo, y, k, P0, w0 = random_shape
    Xg = to_gpu(Xo)
    n_batches = -(-Xo.n // batch)
    c0 = col_counts(Xg.ctx)
    with _env(NFM_COL_LONG=None, NFM_COL_GRID=2):
        auto = train("sgd", Xg, y, k, P0, w0, batch)
    c1 = col_counts(Xg.ctx)
    with _env(NFM_COL_LONG=0, NFM_COL_GRID=2):
        old = train("sgd", Xg, y, k, P0, w0, batch)
    c2 = col_counts(Xg.ctx)
    with _env(NFM_COL_LONG=1, NFM_COL_GRID=2):
        train("sgd", Xg, y, k, P0, w0, batch)
    c3 = col_counts(Xg.ctx)
    assert_same_bits(auto, old, "NFM_COL_LONG unset vs 0")
    # an epoch call enqueues every batch of its plan, or replays the graph of an earlier one: once or EPOCHS times each
    for d in (c1 - c0, c2 - c1, c3 - c2):
        assert d[1] in (n_batches, EPOCHS * n_batches), d
    assert ((c1 - c0)[0] == 0) if batch == 256 else ((c1 - c0)[0] > 0), "NFM_COL_LONG unset: %s" % (c1 - c0)
    assert (c2 - c1)[0] == 0, "NFM_COL_LONG=0: %s" % (c2 - c1)
    assert (c3 - c2)[0] == (c3 - c2)[1], "NFM_COL_LONG=1: %s" % (c3 - c2)
