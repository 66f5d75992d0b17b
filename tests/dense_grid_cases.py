"""The large-grid inputs shared by tests/test_dense_grid_cases.py (CPU) and the GPU suites of the dense solver passes
(tests/test_gpu_pgd.py, tests/test_gpu_katyusha.py through tests/katyusha_cases.py, tests/test_gpu_psgd.py): the smallest
models at which the grid-stride loops of pgd.hip, katyusha.hip and psgd.hip take a second trip, their workgroup partials
outnumber a wavefront, and every k_psgd_step_columns instance runs.  They are not workload shapes: at most 1.05 M doubles per
parameter set.  tests/test_dense_grid_cases.py asserts, from the caps read out of the sources, that each shape still reaches
what it is here for, and the conditions (margins, spread, share of zeros) under which the GPU tolerances carry over.

Every input is a regression task at degree 2 with fitLinear and fitIntercept."""
import functools

import numpy as np

from common import init_fm, random_csr
import pgd_restatement as R

# name -> k, d, samples, entries per sample
SHAPES = {
    "tall": (2, 262300, 48, 24),    # L = 1: rows take a second trip of 156 (two wavefronts and a partial one), da * Kp = 524 600
    "deep": (127, 8201, 48, 24),    # L = 64, Kp = 128 with one padding column: three trips, the last of 9 rows; da * Kp = 1 049 728
    "passes": (33, 16500, 64, 40),  # L = 32, Kp = 64: k_prox_pass_partial's second trip
}
VPT_K, VPT_D = 3, (1500, 6000, 12000, 16384, 16385)  # VPT 2, 8, 16, 16 of k_psgd_step_columns, then the row-parallel path
for _d in VPT_D:
    SHAPES["vpt%d" % _d] = (VPT_K, _d, 64, 40)


def lanes_for_k(k):
    """common.h lanes_for_k"""
    half, L = (k + 1) // 2, 1
    while L < half:
        L <<= 1
    return L


@functools.lru_cache(maxsize=None)
def _data(shape, scale, zero_rows):
    k, d, n, m = SHAPES[shape]
    Xo = random_csr(n, d, m, 17)
    y = np.random.default_rng(18).normal(size=n)
    P0, w0, b0, n_aug = init_fm(d, 2, k, "explicit", True, seed=19, scale=scale)
    # one factor per feature, so that the row norms spread over (0, 2) times their common size: with k = 127 they would
    # otherwise all lie within 6 % of each other and a row operator (L21, SquaredL21) would zero all of them or none
    P0 *= np.random.default_rng(21).uniform(0.0, 2.0, P0.shape[2])
    w0 = np.random.default_rng(20).uniform(-0.1, 0.1, d)
    if zero_rows:  # every other feature starts at zero (tests/katyusha_cases.py says why)
        P0[:, :, ::2] = 0.0
    for a in (P0, w0, y):
        a.setflags(write=False)
    return Xo, y, P0, w0, 0.05, n_aug


def data(shape, scale, zero_rows=False):
    """(Xo, y, P0, w0, b0, n_aug); the arrays are shared between callers and read-only"""
    return _data(shape, scale, zero_rows)


# ---- PGD, FISTA, NMAPGD: name -> (shape, algo, solver keywords, iterations, scale of P0) ----
# gamma is sized so that the prox zeroes between 5 % and 95 % of P at the end of the fit (asserted on the restatement)
PGD_CASES = {
    "tall_pgd_l1": ("tall", "pgd", dict(reg="l1", gamma=1e-2), 3, 0.05),
    "tall_nmapgd_sql12_col": ("tall", "nmapgd", dict(reg="squaredl12", gamma=1e-6), 3, 0.05),
    "tall_fista_sql21": ("tall", "fista", dict(reg="squaredl21", gamma=1e-6), 2, 0.05),
    "deep_nmapgd_l21": ("deep", "nmapgd", dict(reg="l21", gamma=1e-1), 3, 0.05),
    "deep_pgd_sql12_row": ("deep", "pgd", dict(reg="squaredl12", transpose=False, gamma=2e-3), 2, 0.05),
    "deep_fista_sql12_col": ("deep", "fista", dict(reg="squaredl12", gamma=5e-5), 2, 0.05),
}
PGD_BITWISE = ("tall_nmapgd_sql12_col", "deep_nmapgd_l21")


def pgd_inputs(name):
    shape, algo, skw, iters, scale = PGD_CASES[name]
    return data(shape, scale)


@functools.lru_cache(maxsize=None)
def pgd_restate(name, sums="seq"):
    """(solver, result) of the restatement, computed once per process and shared: treat both as read-only"""
    shape, algo, skw, iters, scale = PGD_CASES[name]
    Xo, y, P0, w0, b0, n_aug = pgd_inputs(name)
    s = R.Solver(algo, Xo, y, 2, n_aug, True, True, sums=sums, **skw)
    return s, s.fit(P0, w0, b0, max_iter=iters, tol=0.0)


# ---- MBPSGD, column-wise SquaredL12: name -> (shape, gamma, miniBatchSize, outer iterations); P0 at scale 0.3 ----
# The share of zeros of this operator does not depend on the scale of P (the threshold is homogeneous in it), only on
# gamma * d and on how often the prox is applied.  vpt*: gamma sized for 14 % .. 61 % zeros after eight applications.
# passes: the gamma is given (1e-2); one application leaves 94.8 % zeros, two leave 98 %, so it runs one mini-batch of all 64
# samples once.  passes_finish needs more threshold passes than are enqueued blindly, which only a gamma does that leaves
# next to nothing (34 .. 75 of 544 500 entries survive): it is exempt from the 5 % .. 95 % rule by what it is for.
PSGD_SCALE = 0.3
PSGD_CASES = {"vpt%d" % d: ("vpt%d" % d, 3e-5, 16, 2) for d in VPT_D}
PSGD_CASES["passes"] = ("passes", 1e-2, 64, 1)
PSGD_CASES["passes_finish"] = ("passes", 30.0, 16, 2)  # ends in k_prox_finish


def psgd_stream(n, need, seed=9):
    """tests/test_gpu_psgd.py make_stream"""
    rng = np.random.default_rng(seed)
    out = []
    while sum(len(o) for o in out) < need:
        out.append(rng.permutation(n))
    return np.concatenate(out)[:need].astype(np.int64)


def psgd_oracle(name):
    """the oracle's parameters after the fit tests/test_gpu_psgd.py's check() runs on this case (its configuration, restated)"""
    import oracle as O
    shape, gamma, B, outer = PSGD_CASES[name]
    Xo, y, P0, w0, b0, n_aug = data(shape, PSGD_SCALE)
    inner = (Xo.n - 1) // B + 1
    need = B * inner
    stream = psgd_stream(Xo.n, need * outer)
    cfg = O.psgd_cfg(eta0=0.2, gamma=gamma, beta=1e-2, alpha=1e-2, alpha0=1e-2, reg="squaredl12", transpose=True)
    P, w, b, it = P0.copy(), w0.copy(), b0, 1
    for t in range(outer):
        b, it, _ = O.fm_mbpsgd_epoch(Xo, y, 2, P, w, b, cfg, stream[t * need:(t + 1) * need], B, n_aug, it=it, seed=t + 1)
    return P, w, b


def threshold_passes(v, lam):
    """passes of the deterministic threshold iteration (psgd.hip: tau <- 2 lam sum_{|v_i| > tau} |v_i| / (1 + 2 lam #{|v_i| > tau})
    from 0) until the active count repeats or reaches 0: what k_prox_pass_combine counts per component"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    tau, prev, passes = 0.0, -1, 0
    while True:
        on = a > tau
        c = int(on.sum())
        passes += 1
        if c == prev or c == 0:
            return passes
        tau, prev = 2 * lam * (float(a[on].sum()) / (1.0 + 2.0 * lam * c)), c
