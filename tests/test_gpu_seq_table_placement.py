"""-m gpu: where a one-workgroup kernel keeps its per-sample table changes no bit of a result.

k_sequential (nimfm_amd/csrc/seq.hip) and k_psgd_seq (psgd_seq.hip) choose the table's placement from the dataset's LONGEST
row (ds->max_row), not from the rows an epoch call walks, and both state that the per-thread arithmetic and its order are the
same wherever the table lives (seq.hip's head comment on STAGE; DESIGN.md section 22: every thread on its own column).  So one
dataset of 41 rows and 256 features is built per placement: rows 0..39 are the same in all of them (at most 9 entries, one row
empty, one with a single entry), the last row has L entries and is never visited -- every epoch call covers [0, 40) with an
explicit permutation of 0..39.  P, w, the intercept and the loss and viol sums of two epochs are compared BITWISE across L.

Bytes of LDS asked for (the limit is 160 KB = 163,840 B), from launch_sequential's and psgd_seq_run's own formulas:

degree 3, fitLower = explicit, k = 8: nb = 2, T = 64, no pipelined step (that one takes degree 2 with one order only)
  newSGD / newAdaGrad (mode = sequential)
    L = 9    staged                8 (64 + 2 * 2 * 9 * 64 + 3 * 9)   =  19,160 B
    L = 100  unstaged, dA in LDS   8 (64 + 2 * 100 * 64)             = 102,912 B   (staged: 8 (64 + 4 * 100 * 64 + 300) = 207,712 B)
    L = 200  dA in global memory   8 (64 + 2 * 200 * 64)             = 205,312 B
  newPSGD with newL1() / newL21()
    L = 9    tables in LDS         8 (64 + 263 * 9)                  =  19,448 B
    L = 100  tables in global      8 (64 + 263 * 100)                = 210,912 B

degree 2, k = 200: ONE order, so the kc = 2 blocks of 100 factors are one feature-major row of 2 * 128 factors to this kernel
(seq_row_view): nb = 1, kc = 1, T = 256.  The pipelined step takes such a model while its tables fit, up to L = 38
(8 (256 + 2 * 38 * 256 + 7 * 38) + 1,064 = 160,888 B; L = 39: 163,976 B + 1,092 B), so the three placements start behind it:
    L = 39   staged                8 (256 + 2 * 39 * 256 + 3 * 39)   = 162,728 B
    L = 40   unstaged, dA in LDS   8 (256 + 40 * 256)                =  83,968 B   (staged: 166,848 B)
    L = 80   dA in global memory   8 (256 + 80 * 256)                = 165,888 B   (L = 79: 163,840 B, the limit itself)

degree 3, fitLower = explicit, k = 200: two orders, so the blocks stay blocks: nb = 4, kc = 2, T = 128 -- the kc blocks of one
order continue ONE ascending sum over the factors (sgd.nim:172-173)
    L = 9    staged                8 (128 + 2 * 4 * 9 * 128 + 27)    =  74,968 B
    L = 20   unstaged, dA in LDS   8 (128 + 4 * 20 * 128)            =  82,944 B   (staged: 165,344 B)
    L = 40   dA in global memory   8 (128 + 4 * 40 * 128)            = 164,864 B
"""
import numpy as np
import pytest

import nimfm_amd as nf
from gpu_common import gpu_fm
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
N_WALKED, D, EPOCHS = 40, 256, 2

SOLVERS = {
    "sgd": lambda: nf.newSGD(verbose=0, mode="sequential"),
    "adagrad": lambda: nf.newAdaGrad(verbose=0, mode="sequential"),
    "psgd_l1": lambda: nf.newPSGD(verbose=0, gamma=1e-3, reg=nf.newL1()),
    "psgd_l21": lambda: nf.newPSGD(verbose=0, gamma=1e-3, reg=nf.newL21()),
}


def _rows():
    """rows 0..39 (the same for every L) and the entries a last row of any length is cut from"""
    rng = np.random.default_rng(20240611)
    lengths = rng.integers(2, 10, size=N_WALKED)
    lengths[5], lengths[11], lengths[17] = 0, 1, 9
    rows = []
    for i, m in enumerate(int(v) for v in lengths):
        idx = rng.choice(D, size=m, replace=False)
        if i % 2 == 0:
            idx = np.sort(idx)  # storage order need not be sorted (dataset.nim:597-612)
        rows.append((idx.astype(np.int32), rng.uniform(-1, 1, size=m) / np.sqrt(max(m, 1))))
    return rows, rng.permutation(D).astype(np.int32), rng.uniform(-1, 1, size=D), rng.standard_normal(N_WALKED + 1)


ROWS, LAST_IDX, LAST_VAL, Y = _rows()
PERMS = [np.ascontiguousarray(np.random.default_rng(7 + e).permutation(N_WALKED).astype(np.int64)) for e in range(EPOCHS)]


def _dataset(L):
    rows = ROWS + [(LAST_IDX[:L], LAST_VAL[:L] / np.sqrt(L))]
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    return nf.newCSRDataset(np.concatenate([r[1] for r in rows]), np.concatenate([r[0] for r in rows]), indptr, len(rows), D)


def _start(degree, k):
    rng = np.random.default_rng(99)
    return 0.1 * rng.standard_normal((degree - 1, k, D)), 0.1 * rng.standard_normal(D), 0.05


def _fit(solver, degree, k, L):
    P0, w0, b0 = _start(degree, k)
    X, opt = _dataset(L), SOLVERS[solver]()
    fm = gpu_fm("regression", degree, k, "explicit", True, True, P0, w0, b0)
    fm.init(X)
    X.set_targets(Y)
    opt._handle(fm, X.ctx, "sequential")
    capi.check(capi.lib().nfm_opt_set_it(opt._h, 1))
    if solver.startswith("psgd"):
        capi.check(capi.lib().nfm_psgd_begin_fit(opt._h, X.h))
    sums = [opt._epoch(X, perm, 0, N_WALKED) for perm in PERMS]
    opt._finalize_into(fm)
    return fm.P.copy(), fm.w.copy(), fm.intercept, sums


def _assert_same_bits(solver, degree, k, lengths):
    base = _fit(solver, degree, k, lengths[0])
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
    assert not np.array_equal(base[0], _start(degree, k)[0])  # the walk moved the parameters
    for L in lengths[1:]:
        P, w, b, sums = _fit(solver, degree, k, L)
        what = "%s degree %d k %d: L = %d against L = %d" % (solver, degree, k, L, lengths[0])
        assert np.array_equal(P, base[0]), what
        assert np.array_equal(w, base[1]), what
        assert b == base[2], what
        for (ls, vs), (ls0, vs0) in zip(sums, base[3]):
            assert ls == ls0 and vs == vs0, what


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
def test_sequential_staged_unstaged_and_global_gradient(solver):
    """k_sequential: staged (L = 9), unstaged with dA in LDS (L = 100), dA in global memory (L = 200)"""
    _assert_same_bits(solver, 3, 8, [9, 100, 200])


@pytest.mark.parametrize("solver", ["psgd_l1", "psgd_l21"])
def test_psgd_tables_in_lds_and_global(solver):
    """k_psgd_seq: the tables in LDS (L = 9) and in global memory (L = 100)"""
    _assert_same_bits(solver, 3, 8, [9, 100])


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
def test_sequential_wide_row(solver):
    """k = 200 at degree 2 (one row of 256 factors, T = 256): the three placements behind the pipelined step's reach"""
    _assert_same_bits(solver, 2, 200, [39, 40, 80])


@pytest.mark.parametrize("solver", ["sgd", "adagrad"])
def test_sequential_factor_blocks_continue_one_sum(solver):
    """k = 200 at degree 3 (kc = 2 blocks of 100 factors per order, T = 128): the blocks of an order continue one ascending sum"""
    _assert_same_bits(solver, 3, 200, [9, 20, 40])
