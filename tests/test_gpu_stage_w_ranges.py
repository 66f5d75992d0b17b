"""-m gpu: the linear weights of a batch staged in passes over the entry range (k_stage_w_ranges, NFM_STAGE_W_PASSES=n) against
the gathers they stand in for (bit for bit) and against the mini-batch oracle (oracle/nimfm_mb.c).

Pass p of n takes the entries [p, p + 1) * cap / n of every sample, cap / n lanes per sample, 64 n / cap samples per wavefront
step; it writes the same Wt[pib * cap + q] = w[indices[q0 + q]] as k_stage_w does in feature slices.  Every case trains with
NFM_STAGE_W=1 NFM_STAGE_W_PASSES=n and with NFM_STAGE_W=0, NFM_COL_LONG=1 NFM_COL_GRID=3 as in test_gpu_stage_scalars.py, and
says from the library's launch counters ("stage_w": batches staged, "stage_w_ranges": those staged by the new kernel) which
kernel ran.  The oracle of a dataset is computed once and shared by the pass counts."""
import numpy as np
import pytest

import oracle as O
from common import assert_close, make_perms, random_csr
from gpu_common import _env, ragged_csr, to_gpu
from test_gpu_col_long import assert_same_bits, oracle_train, start, train
from test_gpu_stage_scalars import by_hand

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
N, D, K, B = 3000, 512, 64, 1024  # batches of 1024, 1024 and 952 samples
PASSES = [1, 2, 4, 8, 16]
BASE = dict(NFM_COL_LONG=1, NFM_COL_GRID=3)


def counts(ctx):
    return np.array([ctx.timing_get("stage_w")[0], ctx.timing_get("stage_w_ranges")[0]])


def both_ways(ctx, fn, n, **env):
    """fn() staged in n passes, then gathered; bitwise equal, and every staged batch went through k_stage_w_ranges"""
    kv = dict(BASE)
    kv.update(env)
    c0 = counts(ctx)
    with _env(NFM_STAGE_W=1, NFM_STAGE_W_PASSES=n, **kv):
        new = fn()
    c1 = counts(ctx) - c0
    assert c1[1] > 0 and c1[0] == c1[1], "launches (staged batches, by k_stage_w_ranges) = %s at n = %d" % (c1, n)
    with _env(NFM_STAGE_W=0, NFM_STAGE_W_PASSES=n, **kv):
        old = fn()
    assert (counts(ctx) - c0 == c1).all(), "staging launches with NFM_STAGE_W=0"
    assert_same_bits(new, old, "%d passes vs gathered" % n)
    return new


def against(new, ref):
    assert abs(new["b"][0] - ref["b"]) < 1e-11
    assert_close(new["w"], ref["w"], RTOL, ATOL, "w")
    assert_close(new["P"], ref["P"], RTOL, ATOL, "P")


def case(Xo, y, k, P0, w0, batch, perms=None):
    """a dataset with its start and its oracle result (computed once)"""
    return dict(Xo=Xo, Xg=to_gpu(Xo), y=y, k=k, P0=P0, w0=w0, batch=batch, perms=perms,
                ref=oracle_train("sgd", Xo, y, k, P0, w0, batch, perms, True, 1))


def run(c, n, **env):
    new = both_ways(c["Xg"].ctx, lambda: train("sgd", c["Xg"], c["y"], c["k"], c["P0"], c["w0"], c["batch"], c["perms"], True, 1), n, **env)
    against(new, c["ref"])
    assert not np.array_equal(new["w"], c["w0"])


def sorted_rows(lengths, d, seed):
    """rows of the given lengths, ids distinct and ascending: (a + b t) mod d for t < length with b odd, d a power of two"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n, m = len(lengths), int(lengths.max())
    a, b = rng.integers(0, d, (n, 1)), 2 * rng.integers(0, d // 2, (n, 1)) + 1
    ids = (a + b * np.arange(m)) % d
    keep = np.arange(m) < lengths[:, None]
    ids = np.sort(np.where(keep, ids, d), axis=1)  # a row's own ids first, ascending
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    return O.Dataset(indptr, ids[keep], rng.uniform(-1, 1, int(indptr[-1])), n, d)


@pytest.fixture(scope="module")
def full_rows():
    Xo = random_csr(N, D, 64, seed=41)
    y = np.random.default_rng(42).standard_normal(N)
    return case(Xo, y, K, *start(D, K, 43), B)


@pytest.mark.parametrize("n", PASSES + [64])
def test_full_rows(full_rows, n):
    """rows of 64 entries: the row phase holds 64 per sample; n = 64 is one lane per sample"""
    assert full_rows["Xg"].rows_ascend()
    run(full_rows, n)


@pytest.fixture(scope="module")
def short_rows():
    """k = 13 at one row slot: 8 lanes hold 32 entries per sample, two samples per wavefront in k_row_phase and a stride of 32 in
    Wt.  Rows of 0 ... 32 entries, so at every n < 32 some sample takes several lane groups of a wavefront step."""
    lengths = np.random.default_rng(44).integers(0, 33, N)
    lengths[:8] = [32, 0, 1, 32, 31, 17, 32, 2]
    Xo = sorted_rows(lengths, D, 45)
    y = np.random.default_rng(46).standard_normal(N)
    return case(Xo, y, 13, *start(D, 13, 47), B)


@pytest.mark.parametrize("n", PASSES + [32])
def test_capacity_32(short_rows, n):
    run(short_rows, n, NFM_SPLIT=1)


def test_capacity_32_refuses_64_passes(short_rows):
    c = short_rows
    with _env(NFM_STAGE_W=1, NFM_STAGE_W_PASSES=64, NFM_SPLIT=1, **BASE):
        with pytest.raises(ValueError, match="NFM_STAGE_W_PASSES"):
            train("sgd", c["Xg"], c["y"], c["k"], c["P0"], c["w0"], c["batch"])


def test_capacity_32_by_the_batch_size():
    """the one-slot mapping chosen by choose_split itself: 8 lanes per row and a batch of 32768 samples ask for one slot on a
    chip of 256 compute units (fewer units: fewer slots still).  Two batches, the second short."""
    n, batch = 32768 + 1001, 32768
    lengths = np.random.default_rng(48).integers(0, 33, n)
    Xo = sorted_rows(lengths, D, 49)
    y = np.random.default_rng(50).standard_normal(n)
    run(case(Xo, y, 13, *start(D, 13, 51), batch), 4)


@pytest.fixture(scope="module")
def ragged_rows():
    Xo = ragged_csr(N, D, seed=52, max_m=64, empty_every=7)
    lens = np.diff(Xo.indptr)
    assert lens.min() == 0 and lens.max() == 64 and (lens[3::7] == 0).all()
    y = np.random.default_rng(53).standard_normal(N)
    return case(Xo, y, K, *start(D, K, 54), B)


@pytest.mark.parametrize("n", PASSES)
def test_ragged_rows_with_empty_samples(ragged_rows, n):
    """rows of 0 ... 64 entries, every seventh empty (every other one stored unsorted: the knob forces the kernel)"""
    run(ragged_rows, n)


@pytest.mark.parametrize("n,lengths", [(4, (15, 16, 17)), (8, (7, 8, 9))])
def test_rows_that_end_at_a_pass_boundary(n, lengths):
    """one short of, on and one past the first pass's last entry (64 / n per pass); the rows begin at CSR offsets 0, 15, 31, 48 ...
    (0, 7, 15, 24 ...), so a pass's 64-byte (32-byte) piece of a row's ids is rarely aligned"""
    Xo = sorted_rows(np.resize(lengths, N), D, 55 + n)
    assert (Xo.indptr[1:7] % 16 != 0).sum() >= 4
    y = np.random.default_rng(56).standard_normal(N)
    c = case(Xo, y, K, *start(D, K, 57), B)
    for m in sorted({n, 4, 8}):
        run(c, m)


@pytest.fixture(scope="module")
def unsorted_rows():
    Xo = random_csr(N, D, 24, seed=58, sorted_idx=False)
    assert (np.diff(Xo.indices.reshape(N, 24), axis=1) < 0).any()
    y = np.random.default_rng(59).standard_normal(N)
    return case(Xo, y, K, *start(D, K, 60), B)


@pytest.mark.parametrize("n", PASSES)
def test_rows_stored_unsorted_forced(unsorted_rows, n):
    """the knob takes the new kernel whatever the rows look like: the same table, only the locality is lost"""
    assert not unsorted_rows["Xg"].rows_ascend()
    run(unsorted_rows, n)


def test_knob_unset_goes_by_the_rows(unsorted_rows, full_rows):
    """NFM_STAGE_W_PASSES unset: slices (k_stage_w) where some row descends, entry ranges where every row ascends; 0: slices"""
    for c, knob, ranges in ((unsorted_rows, None, False), (full_rows, None, True), (full_rows, 0, False)):
        ctx = c["Xg"].ctx
        c0 = counts(ctx)
        with _env(NFM_STAGE_W=1, NFM_STAGE_W_PASSES=knob, **BASE):
            new = train("sgd", c["Xg"], c["y"], c["k"], c["P0"], c["w0"], c["batch"])
        c1 = counts(ctx) - c0
        assert c1[0] > 0 and c1[1] == (c1[0] if ranges else 0), "launches (staged batches, by k_stage_w_ranges) = %s" % c1
        against(new, c["ref"])


@pytest.fixture(scope="module")
def permuted(full_rows):
    c = full_rows
    return case(c["Xo"], c["y"], K, c["P0"], c["w0"], B, perms=make_perms(N, 2))


@pytest.mark.parametrize("n", PASSES)
def test_host_permutation(permuted, n):
    run(permuted, n)


@pytest.mark.parametrize("n", PASSES)
def test_device_drawn_order(full_rows, n):
    c = full_rows
    new = both_ways(c["Xg"].ctx, lambda: by_hand(c["Xg"], c["y"], K, c["P0"], c["w0"], B, [(0, N)] * 2, seed=7), n)
    P, w, b, it = c["P0"].copy(), c["w0"].copy(), 0.0, 1
    for e in range(2):
        b, it, ls, vs = O.fm_sgd_epoch_mb(c["Xo"], c["y"], 2, P, w, b, O.sgd_cfg(), B, perm=new["perms"][e].astype(np.int64), it=it)
        assert_close([ls, vs], [new["loss"][e], new["viol"][e]], 1e-9, 0, "loss / viol of epoch %d" % e)
    against(new, {"P": P, "w": w, "b": b})


@pytest.fixture(scope="module")
def sub_range_oracle(full_rows):
    c = full_rows
    calls = [(0, 700), (700, 2950), (2950, N)]
    P, w, b, it, sums = c["P0"].copy(), c["w0"].copy(), 0.0, 1, []
    for lo, hi in calls:
        b, it, ls, vs = O.fm_sgd_epoch_mb(c["Xo"], c["y"], 2, P, w, b, O.sgd_cfg(), B, begin=lo, end=hi, it=it)
        sums.append((ls, vs))
    return calls, sums, {"P": P, "w": w, "b": b}


@pytest.mark.parametrize("n", PASSES)
def test_sub_range_calls(full_rows, sub_range_oracle, n):
    """three epoch calls over consecutive ranges: every call's first batch stages from the w the previous call left"""
    c = full_rows
    calls, sums, ref = sub_range_oracle
    new = both_ways(c["Xg"].ctx, lambda: by_hand(c["Xg"], c["y"], K, c["P0"], c["w0"], B, calls), n)
    for i, (lo, hi) in enumerate(calls):
        assert_close(sums[i], [new["loss"][i], new["viol"][i]], 1e-9, 1e-12, "loss / viol of [%d, %d)" % (lo, hi))
    against(new, ref)


@pytest.fixture(scope="module")
def odd_batches():
    """batches of 1021, 1021 and 957 samples: no multiple of the 2 ... 16 samples of a wavefront step, ragged rows"""
    n = 2999
    Xo = sorted_rows(np.random.default_rng(61).integers(0, 65, n), D, 62)
    y = np.random.default_rng(63).standard_normal(n)
    return case(Xo, y, K, *start(D, K, 64), 1021)


@pytest.mark.parametrize("n", PASSES + [32, 64])
def test_batch_that_ends_inside_a_wavefront_step(odd_batches, n):
    assert all(s % 2 for s in (1021, 2999 - 2 * 1021))
    run(odd_batches, n)


def test_graph_replay(full_rows):
    """12 batches of 256: the first epoch call captures the launches as a graph, the second replays it"""
    c = dict(full_rows, batch=256)
    c["ref"] = oracle_train("sgd", c["Xo"], c["y"], K, c["P0"], c["w0"], 256, None, True, 1)
    run(c, 4)


def test_rows_ascend_flag(full_rows, ragged_rows, short_rows):
    """true for a sorted dataset (empty and one-entry rows included), false when one row has one descending pair"""
    assert full_rows["Xg"].rows_ascend() and short_rows["Xg"].rows_ascend()
    assert not ragged_rows["Xg"].rows_ascend()
    Xo = full_rows["Xo"]
    idx = Xo.indices.copy()
    q = 1234 * 64 + 30
    idx[q], idx[q + 1] = idx[q + 1], idx[q]
    assert not to_gpu(O.Dataset(Xo.indptr, idx, Xo.data, N, D)).rows_ascend()
    one = to_gpu(O.Dataset(np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64) % D, np.ones(N), N, D))
    assert one.rows_ascend()
