"""-m gpu: every route of a sequential-mode call (nimfm_amd/csrc/seq_route.h) is reached by the smallest shape that takes it, and
the library says so: one counter per route (seq_route_win_* for the window's four workers, seq_route_pipe / _pipe_wide / _staged /
_plain / _plain_scratch for the one-workgroup kernels), bumped once per epoch call with timing on or off.  Each case makes ONE
epoch call and asserts that exactly the counter tests/seq_route_cases.py predicts for its shape went up by one and no other
seq_route_* moved, and that the fit equals the NFM_SEQ_WIN=0 fit: bit for bit, or at rtol 1e-8 / atol 1e-11 where the window's
one-term chain ran (a fitted intercept: tests/test_gpu_seqwin.py's rule for that flavour).

512 samples, at most 64 features and 8 entries per row, except the table-in-scratch case: its route needs ONE row of 330 entries
at 64 factors (168,960 bytes of per-sample table do not fit a CU's LDS)."""
import numpy as np
import pytest

import nimfm_amd as nf
import oracle as O
import seq_route_cases as C
from common import assert_close, init_ffm, init_fm
from gpu_common import _env, gpu_ffm, gpu_fm, to_gpu

pytestmark = pytest.mark.gpu

N = 512
COUNTERS = ["seq_route_win_" + w for w in C.WORKERS] + ["seq_route_pipe", "seq_route_pipe_wide", "seq_route_staged", "seq_route_plain",
                                                        "seq_route_plain_scratch"]
# name: (model, factors, fields or degree, features, longest row); "fm": one order of degree 2; "fmx": degree 3 with its lower order
WINDOW = {"k64": ("fm", 64, 2, 64, 8), "general": ("fm", 8, 2, 40, 8), "fmx": ("fmx", 8, 3, 40, 8), "ffm": ("ffm", 4, 3, 30, 6)}
# 8 factors, 8 entries: one row per thread | 8 fields x 8 entries at 32 factors: 8 rows per thread of 256, so 512 threads |
# two orders: no pipelined step, the staged one | 33 fields x 8 entries at 64 factors: 66 rows per thread, no stage for fields |
# one row of 330 entries at 64 factors: the table in global scratch
ONE_WG = {"pipe": ("fm", 8, 2, 40, 8), "pipe_wide": ("ffm", 32, 8, 64, 8), "staged": ("fmx", 8, 3, 40, 8), "plain": ("ffm", 64, 33, 64, 8),
          "plain_scratch": ("fm", 64, 2, 400, 330)}


def data(model, F, d, max_m, seed):
    """rows of 1 ... max_m entries (the first one: max_m, so the longest row is known), a few empty; fields for "ffm" """
    rng = np.random.default_rng(seed)
    lens = [max_m] + [0 if i % 13 == 5 else int(rng.integers(1, min(max_m, 8) + 1)) for i in range(1, N)]
    rows = [np.sort(rng.choice(d, size=m, replace=False)) for m in lens]
    idx = np.concatenate(rows).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = rng.uniform(-1, 1, len(idx)) * (0.1 if max_m > 64 else 1.0)
    y = rng.standard_normal(N)
    if model == "ffm":
        return O.Dataset(indptr, idx, vals, N, d, rng.integers(0, F, size=d)[idx], F), y
    return O.Dataset(indptr, idx, vals, N, d), y


def shape(model, k, F, d, max_m, fit_intercept, kind):
    a = dict(m_cap=max_m, fit_intercept=int(fit_intercept), ada=int(kind == "adagrad"), ns=N, d=d)
    return C.ffm_shape(k, F, **a) if model == "ffm" else C.fm_shape(k, degree=F, orders=F - 1, **a)


def one_call(case, kind, fit_intercept, seed, **env):
    """one epoch call under env -> (P, w, b, AdaGrad's state or None, {counter: how often it went up})"""
    model, k, F, d, max_m = case
    Xo, y = data(model, F, d, max_m, seed)
    if model == "ffm":
        P0, w0, b0 = init_ffm(d, F, k, seed=seed)
        m = gpu_ffm("regression", k, True, fit_intercept, P0, w0, b0)
    else:
        P0, w0, b0, n_aug = init_fm(d, F, k, "explicit", True, seed=seed)
        assert n_aug == 0
        m = gpu_fm("regression", F, k, "explicit", True, fit_intercept, P0, w0, b0)
    opt = (nf.newSGD if kind == "sgd" else nf.newAdaGrad)(maxIter=1, verbose=0, tol=0, shuffle=False, mode="sequential",
                                                          **(dict(eta0=0.02) if kind == "sgd" else {}))
    ctx = nf.default_context()
    with _env(NFM_SEQ_WIN_EXACT=None, NFM_SEQ_WIN_NOCOND=None, NFM_SEQ_WIN_W=None, NFM_SEQ_WIN_PAR=None, **env):
        before = {c: ctx.timing_get(c)[0] for c in COUNTERS + ["seq_window_launch", "seq_window_fallback"]}
        opt.fit(to_gpu(Xo), y, m)
        went_up = {c: ctx.timing_get(c)[0] - n for c, n in before.items()}
    assert went_up.pop("seq_window_fallback") == 0, "a window launch aborted"
    return m.P.copy(), m.w.copy(), m.intercept, opt.get_state(m) if kind == "adagrad" else None, went_up


def same_fit(got, ref, bitwise, what):
    arrays = [("P", got[0], ref[0]), ("w", got[1], ref[1]), ("b", got[2], ref[2])]
    if got[3] is not None:
        arrays += [(n, g, h) for n, g, h in zip(["g_sum.P", "g_norm.P", "g_sum.w", "g_norm.w", "g_sum.b", "g_norm.b"], got[3], ref[3])]
    for name, a, b in arrays:
        a, b = np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64)), np.atleast_1d(np.ascontiguousarray(b, dtype=np.float64))
        if bitwise:
            assert a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all(), (what, name, np.abs(a - b).max())
        else:
            assert_close(a, b, 1e-8, 1e-11, "%s %s" % (what, name))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
@pytest.mark.parametrize("fit_intercept", [True, False])
@pytest.mark.parametrize("worker", list(WINDOW))
def test_the_window_counts_the_worker_it_launched(worker, fit_intercept, kind):
    case = WINDOW[worker]
    want = C.win_route(shape(*case, fit_intercept, kind), C.Knobs(win=2))
    assert want["offered"] and want["fits"] and want["worker"] == worker and want["one_term"] == int(fit_intercept), want
    ref = one_call(case, kind, fit_intercept, seed=3, NFM_SEQ_WIN=0)
    win = one_call(case, kind, fit_intercept, seed=3, NFM_SEQ_WIN=2)
    assert win[4].pop("seq_window_launch") >= 1 and ref[4].pop("seq_window_launch") == 0
    assert win[4] == {c: int(c == want["counter"]) for c in COUNTERS}, (want["counter"], win[4])
    assert sum(ref[4].values()) == 1 and not any(v for c, v in ref[4].items() if c.startswith("seq_route_win_")), ref[4]
    same_fit(win, ref, bitwise=not want["one_term"], what=worker)


@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
@pytest.mark.parametrize("route", list(ONE_WG))
def test_the_one_workgroup_kernels_count_the_step_they_launched(route, kind):
    case = ONE_WG[route]
    S = shape(*case, True, kind)
    assert not C.win_route(S, C.Knobs())["offered"]  # 512 samples: the window is not worth its snapshot
    want = C.one_wg_route(C.row_view(S), C.Knobs())
    assert want["counter"] == "seq_route_" + route, want
    ref = one_call(case, kind, True, seed=5, NFM_SEQ_WIN=0)
    got = one_call(case, kind, True, seed=5, NFM_SEQ_WIN=None)
    for r in (ref, got):
        assert r[4].pop("seq_window_launch") == 0
        assert r[4] == {c: int(c == want["counter"]) for c in COUNTERS}, (want["counter"], r[4])
    same_fit(got, ref, bitwise=True, what=route)
    assert not np.array_equal(got[0], init_ffm(case[3], case[2], case[1], seed=5)[0] if case[0] == "ffm" else
                              init_fm(case[3], case[2], case[1], "explicit", True, seed=5)[0]), "the call did not train"
