"""The inputs shared by tests/test_row_slot_cases.py (CPU) and tests/test_gpu_row_slots.py: data sets with explicit row lengths,
the table of (k, requested row slots, data set, regime, solver, model) cases, and a restatement of what the host chooses for
each of them -- which k_row_phase<L, SPLIT, OPT, GEN, MODE, SING> a mini-batch takes, which decisionFunction kernel a call.

choose_split (csrc/lane_map.h) gives a small launch min(64/L, 16) row slots per sample, so shapes of a few hundred samples
run only the largest SPLIT of each L.  NFM_SPLIT (read per call, inside choose_split) puts them on every other lane mapping; the
restatement below says which one a request ends at, tests/test_row_slot_cases.py asserts that the table reaches all of them.

Every function that restates host code names the function it restates; tests/test_cpp_mb_route.py runs the row-phase half
against csrc/mb_route.h itself."""
import collections
import functools

import numpy as np

kWave = 64
SHORT = [0, 1, 2, 7, 8, 9, 16, 31, 32]  # the longest row is exactly one chunk of 32 held entries
LONG = SHORT + [33, 63, 64, 65, 127, 128, 129, 150]  # either side of one and of two chunks of 32 and of 64
FAMILIES = {"short": SHORT, "long": LONG}
EDGE_LENGTHS = (31, 32, 33, 64, 65)  # what the first and the last batch of an epoch must both hold (of the family's lengths)
N_TRAIN, N_PREDICT = 700, 261
# regime -> (d, batch).  dense: batches of 301, 301 and 98 (AdaGrad's first epoch: 1, 301, 301, 97), none a multiple of 4, so
# every samples-per-block count from 4 to 256 ends inside a block; lambda = batch * mean row / d is far above 1.4: no singles.
# sparse: lambda <= 1.4, most features of a batch are touched once and updated by the row phase itself.
REGIMES = {"dense": (200, 301), "sparse": (30000, 129)}
KS = (1, 3, 7, 13, 30, 50)  # L = 1, 2, 4, 8, 16, 32, every one with padding lanes (k odd or below 2 L)
# model -> (degree, fitLower, fitLinear)
MODELS = {
    "deg2": (2, "explicit", True),
    "deg2_nolin": (2, "explicit", False),
    "deg2_aug": (2, "augment", False),  # one dummy feature every sample touches: m_tot = m + 1 crosses 32 and 64
    # no interaction block: the one model the held lane mappings stream (MODE 0 at L * SPLIT >= 8).  On the long rows: a lane adds up
    # every (L * SPLIT)-th entry, so on rows of at most 32 entries 32 and 64 lanes per sample are the same sum
    "deg1": (1, "explicit", True),
    "deg3_explicit": (3, "explicit", True),  # two orders (GEN)
    "deg3_augment": (3, "augment", True),  # one order of degree 3 and a dummy feature (GEN)
}
# (data set, regime, model) per k, each for SGD and AdaGrad
GROUPS = [("short", "dense", "deg2"), ("long", "dense", "deg2_nolin"), ("short", "sparse", "deg2"), ("long", "sparse", "deg2_aug"),
          ("long", "dense", "deg1")]
GEN_KS = (7, 13)
GEN_GROUPS = [("short", "dense", "deg3_explicit"), ("long", "dense", "deg3_augment")]
MBPSGD_GROUP = (13, "long", "dense", "deg2")
# decisionFunction: model -> (degree, fitLower); the linear term is always fitted there
PREDICT_MODELS = {"deg2": (2, "explicit"), "deg3_none": (3, "none"), "deg3_explicit": (3, "explicit"), "deg4_explicit": (4, "explicit"),
                  "deg3_augment": (3, "augment")}

Case = collections.namedtuple("Case", "k request family regime solver model")


# ---------------------------------------------------------------- data
class Csr:
    def __init__(self, indptr, indices, data, n, d):
        self.indptr, self.indices, self.data, self.n, self.d = (np.asarray(indptr, np.int64), np.asarray(indices, np.int64),
                                                                np.asarray(data, np.float64), n, d)

    def lengths(self):
        return np.diff(self.indptr)


N_HUBS = 16


def lengths_csr(lengths, n, d, seed, hubs=0):
    """n rows, row i of lengths[(i - 1) % len(lengths)] entries (row 0 is the longest: AdaGrad's parameters are a function of its
    state, which starts at zero, and only its first step, a mini-batch of one sample, reads the stored ones -- from an empty
    first row P would stay zero for good, and from a short one most of a model of degree 3) with distinct column ids and values
    from U(-1, 1); every other row (the odd ones) is stored unsorted.
    hubs > 0: two entries of every row of two or more come from the first `hubs` ids, the others from the rest -- where d is
    far above the number of entries of an epoch, the popular ids are what carries a nonzero state from sample to sample."""
    rng = np.random.default_rng(seed)
    rows, vals, indptr = [], [], [0]
    for i in range(n):
        m = lengths[(i - 1) % len(lengths)]
        if hubs and m >= 2:
            idx = np.sort(np.concatenate([rng.choice(hubs, size=2, replace=False), hubs + rng.choice(d - hubs, size=m - 2, replace=False)]))
        else:
            idx = np.sort(hubs + rng.choice(d - hubs, size=m, replace=False))
        if i % 2 and m >= 2:
            idx = rng.permutation(idx)
            if np.all(np.diff(idx) > 0):
                idx = idx[::-1]
        rows.append(idx)
        vals.append(rng.uniform(-1, 1, size=m))
        indptr.append(indptr[-1] + m)
    return Csr(indptr, np.concatenate(rows), np.concatenate(vals), n, d)


@functools.lru_cache(maxsize=None)
def _data(family, d, n):
    X = lengths_csr(FAMILIES[family], n, d, seed=[len(family), d, n], hubs=N_HUBS if d == REGIMES["sparse"][0] else 0)
    y = np.random.default_rng(n).standard_normal(n)
    for a in (X.indptr, X.indices, X.data, y):
        a.setflags(write=False)
    return X, y


def train_data(family, regime):
    """(Csr, y): shared between callers and read-only"""
    return _data(family, REGIMES[regime][0], N_TRAIN)


def predict_data(family="long"):
    return _data(family, REGIMES["dense"][0], N_PREDICT)[0]


@functools.lru_cache(maxsize=None)
def train_perms(family, regime):
    """the orders of the two epochs: the data set's own order in the dense regime (None), fixed permutations in the sparse one.
    The first epoch's starts with a row of two entries, both popular ids: AdaGrad's first mini-batch is that one sample
    (plan.hip:1039) and goes through k_row_phase whatever route the others take (see signature())."""
    if regime == "dense":
        return None
    X, _ = train_data(family, regime)
    rng = np.random.default_rng(7)
    perms = np.stack([rng.permutation(X.n) for _ in range(2)]).astype(np.int64)
    at = int(np.flatnonzero(X.lengths()[perms[0]] == 2)[0])
    perms[0, [0, at]] = perms[0, [at, 0]]
    perms.setflags(write=False)
    return perms


def batches(n, batch, first_singleton):
    """[(begin, end)] positions of an epoch's mini-batches (plan.hip:1039: AdaGrad's very first step is a batch of its own)"""
    cuts = [0] + ([1] if first_singleton and n > 0 else [])
    while cuts[-1] < n:
        cuts.append(min(cuts[-1] + batch, n))
    return list(zip(cuts[:-1], cuts[1:]))


# ---------------------------------------------------------------- the model's shape (oracle/nimfm_oracle.c:91-99)
def n_orders(degree, fit_lower):
    return 0 if degree == 1 else (degree - 1 if fit_lower == "explicit" else 1)


def n_augments(degree, fit_lower, fit_linear):
    return (degree - 2 if fit_linear else degree - 1) if fit_lower == "augment" else 0


def lanes_for_k(k):
    """lanes_for_k, common.h"""
    half, L = (k + 1) // 2, 1
    while L < half:
        L <<= 1
    return L


# ---------------------------------------------------------------- the slot count
def p2(v):
    """p2 inside choose_split, lane_map.h"""
    r = 1
    while r < v and r < 64:
        r <<= 1
    return r


def requested_split(L, request):
    """the NFM_SPLIT branch of choose_split (lane_map.h) for a request >= 1"""
    R = kWave // L
    return R if request > R else (16 if request > 16 else p2(request))


def ladder(split, R, rungs=(16, 8, 4, 2)):
    """the rungs that turn choose_split's answer into a template argument: row_slots (mb_route.h), launch_fm_predict
    (predict.hip); launch_fm_predict_orders (predict.hip) with rungs (8, 4, 2)"""
    for r in rungs:
        if R >= r and split >= r:
            return r
    return 1


def row_slots(L, request):
    """SPLIT of the row phase and of k_fm_predict for NFM_SPLIT=request: min(p2(request), 64 / L, 16)"""
    return ladder(requested_split(L, request), kWave // L)


def slot_counts(L):
    return [s for s in (1, 2, 4, 8, 16) if s <= kWave // L]


def requests(L):
    """every power of two up to min(64 / L, 16) and one request beyond: 16 where 64 / L < 16, 64 where L <= 4"""
    return slot_counts(L) + [16 if kWave // L < 16 else 64]


PAIRS = [(L, s) for L in (1, 2, 4, 8, 16, 32) for s in slot_counts(L)]  # the 24 lane mappings with L <= 32


# ---------------------------------------------------------------- the row phase
def held_entries(L, s):
    """E: held_entries (mb_route.h)"""
    lps = L * s
    return 1 if lps >= kWave else (min(kWave // lps, 4) if lps >= 8 else 0)


def held_capacity(L, s):
    """CAP = E * L * SPLIT: held_capacity (mb_route.h)"""
    return held_entries(L, s) * L * s


def use_singles(solver, degree, nb, batch, nnz, n, d):
    """api.hip:1768-1769"""
    lam = batch * (nnz / max(n, 1)) / d
    return solver != "mbpsgd" and degree == 2 and nb == 1 and (batch == 1 or lam <= 1.4)


def mode_for(L, s, sgd, gen, singles, nb, max_row_tot):
    """route_detail::row_mode (mb_route.h) with NFM_HELD and NFM_NQ unset"""
    if held_capacity(L, s) == 0 or nb == 0:
        return 0
    if max_row_tot > held_capacity(L, s):
        return 3
    if not gen and sgd and singles and L * s == kWave:
        return 2
    return 1


def launch_row(L, s, sgd, gen, mode, singles):
    """(MODE, SING) of the k_row_phase instance: MbRoute::mode and sing (mb_route), launch_row (mb_fm_kernels.h).  MODE 2 stands for
    2 and 4: 4 is 2 with streamed stores, for tables beyond 384 MB (kStreamTableBytes), the same code otherwise."""
    can_hold = held_entries(L, s) > 0
    can_reg = can_hold and not gen and sgd and L * s == kWave
    if can_reg and mode == 2:
        return 2, False
    if can_hold and mode == 3:
        return 3, False
    if can_hold and mode >= 1:
        return 1, False
    return 0, bool(singles and not gen)


def takes_ada2(L, solver, gen, singles, stored, max_row_tot):
    """route_detail::ada2_shape and mb_route (mb_route.h) with NFM_ADA2 unset: two wavefronts per sample, whatever choose_split said"""
    return solver == "adagrad" and not gen and L == 32 and singles and not stored and max_row_tot <= 64


Path = collections.namedtuple("Path", "kernel L slots mode sing singles gen stored held cap samples widest b first")  # b: the batch's index in its epoch; first: AdaGrad's first epoch


def fit_paths(case, epochs=2):
    """one Path per mini-batch of a fit of `epochs` epochs from it = 1: the kernel its row phase runs"""
    X, _ = train_data(case.family, case.regime)
    d, batch = REGIMES[case.regime]
    degree, fit_lower, fit_linear = MODELS[case.model]
    nb, n_aug = n_orders(degree, fit_lower), n_augments(degree, fit_lower, fit_linear)
    gen = not (nb == 1 and degree == 2)  # mb_fm.hip:125
    L = lanes_for_k(case.k)
    s = row_slots(L, case.request)
    singles = use_singles(case.solver, degree, nb, batch, len(X.data), X.n, d)
    max_row_tot = int(X.lengths().max()) + n_aug
    perms = train_perms(case.family, case.regime)
    out = []
    for e in range(epochs):
        order = np.arange(X.n) if perms is None else perms[e]
        # the batch that reads the stored parameters: MbRoute::use_stored
        first = case.solver == "adagrad" and e == 0
        cuts = batches(X.n, batch, first)
        if case.solver == "mbpsgd":  # (X.n - 1) // batch + 1 full mini-batches cut from a stream that wraps
            cuts = [(0, batch)] * ((X.n - 1) // batch + 1)
        for b, (lo, hi) in enumerate(cuts):
            stored = case.solver == "mbpsgd" or (first and b == 0)
            widest = max_row_tot if case.solver == "mbpsgd" else int(X.lengths()[order[lo:hi]].max()) + n_aug
            if takes_ada2(L, case.solver, gen, singles, stored, max_row_tot):
                out.append(Path("ada2", L, 2, None, False, True, gen, stored, 1, 64, hi - lo, widest, b, first))
                continue
            mode = mode_for(L, s, case.solver == "sgd", gen, singles, nb, max_row_tot)
            m, sing = launch_row(L, s, case.solver == "sgd", gen, mode, singles)
            out.append(Path("row", L, s, m, sing, singles, gen, stored, held_entries(L, s), held_capacity(L, s), hi - lo, widest, b, first))
    return out


def signature(case):
    """what of the request can reach the result: per mini-batch the kernel and the slot count.  Two requests with one signature
    must give the same bits, two with different signatures different ones.  The slot count is left out of a batch whose widest
    row gives the slots nothing to add up in another order: at most one entry; or two entries at L = 32, AdaGrad's first step
    here -- with one slot and with two the entries sit in lanes 0 and 1 of the sample, every sum over the row has two terms, and
    the lanes a second slot adds hold zeros."""
    def still(p):
        return p.widest <= 1 or (p.widest <= 2 and p.L == 32)
    return tuple((p.kernel, p.mode, p.sing, p.slots if p.kernel == "row" and not still(p) else 0) for p in fit_paths(case))


def stage_w_cap(case):
    """the stride of the k_stage_w table where NFM_STAGE_W=1 stages a batch's linear weights, else 0: SGD, one order of degree
    2, a fitted linear term, MODE 1 (route_detail::may_stage_w and MbRoute::w_cap, mb_route.h; the buffer: mb_work_bounds)"""
    degree, fit_lower, fit_linear = MODELS[case.model]
    p = fit_paths(case)[0]
    return p.cap if case.solver == "sgd" and not p.gen and fit_linear and p.mode == 1 else 0


# ---------------------------------------------------------------- decisionFunction
def predict_kernel(k, request, model, X=None):
    """("orders", LT, SPLIT) where k_interleave_orders + k_fm_predict_orders<LT, SPLIT> take the call (predict.hip:182-189 with
    NFM_PREDICT_ORDERS unset, :171-178 -- the floor of two slots does not apply while NFM_SPLIT is set), else
    ("predict", L, SPLIT) for k_fm_predict<L, SPLIT> (:286-291)"""
    X = predict_data() if X is None else X
    degree, fit_lower = PREDICT_MODELS[model]
    nb, n_aug = n_orders(degree, fit_lower), n_augments(degree, fit_lower, True)
    L = lanes_for_k(k)
    if nb >= 2:
        LT = p2(nb) * L
        if LT <= kWave and len(X.data) + n_aug * X.n >= 2 * (X.d + n_aug):
            return "orders", LT, ladder(requested_split(LT, request), kWave // LT, (8, 4, 2))
    return "predict", L, row_slots(L, request)


# ---------------------------------------------------------------- the table
def groups():
    """[(k, family, regime, solver, model)]: one oracle run and one GPU test id each"""
    out = [(k, f, r, s, m) for k in KS for (f, r, m) in GROUPS for s in ("sgd", "adagrad")]
    out += [(k, f, r, s, m) for k in GEN_KS for (f, r, m) in GEN_GROUPS for s in ("sgd", "adagrad")]
    k, f, r, m = MBPSGD_GROUP
    return out + [(k, f, r, "mbpsgd", m)]


def cases_of(group):
    k, f, r, s, m = group
    return [Case(k, q, f, r, s, m) for q in requests(lanes_for_k(k))]


def table():
    return [c for g in groups() for c in cases_of(g)]
