"""The inputs shared by tests/test_cd_schedule_cases.py (CPU) and the schedule-edge tests of tests/test_gpu_cd.py,
tests/test_gpu_pcd.py and tests/test_gpu_pbcd.py: matrices whose level schedule and run schedule are chosen by construction,
at the widths and column lengths where cd.hip and pbcd.hip take another path.

A *banded one-hot* matrix has m groups of consecutive feature ids; every sample holds exactly one feature of every group
(rows are sorted), values are drawn from +-[0.5, 1.5] and every feature is used at least once.  Group g is then exactly level
g + 1 of the level schedule and exactly run g of the run schedule; the widths are the group sizes and the column lengths are
the per-feature sample counts.  A group is an int (its width: the samples are dealt out evenly) or a list (its features'
column lengths, which sum to n).

gaps = True doubles every column id, so an empty column follows every feature, and puts pad[g] further unused ids behind group g.
Empty columns are level 0 -- one level of their own, ahead of all others -- and join the run they follow, so run g is
2 * width + pad[g] features wide.  Doubling alone makes every run even but the last: the pads are what lets a run of 63, one of
64 and one of 65 stand in one matrix.

tests/test_cd_schedule_cases.py asserts, from the constants read out of the sources, what each case is here for."""
import functools

import numpy as np

from common import init_fm

LENGTHS = [63, 64, 65, 1, 129]  # column lengths either side of a wavefront, a single entry, and two chunks and one entry

# name -> n, groups, gaps, pad
CASES = {
    # launches: narrow [63], wide 64, wide 65, narrow [1, 16, 17, 15], wide 130, narrow [5]
    "edges": dict(n=322, groups=[63, 64, 65, 1, 16, 17, 15, 130, LENGTHS]),
    # levels: wide (the 331 empty columns), narrow [31, 32, 32, 1, 16, 17, 63], wide 64, wide 65, narrow [5]
    # runs: narrow [63], wide 64, wide 65, narrow [2, 32, 34], wide 126, wide 128, wide 130, narrow [13]
    "edges_gaps": dict(n=322, groups=[31, 32, 32, 1, 16, 17, 63, 64, 65, LENGTHS], gaps=True, pad=[1, 0, 1, 0, 0, 0, 0, 0, 0, 3]),
    # n = 2 * 1024 + 2: the sums over every sample take two full trips and a partial one
    "long_1025": dict(n=2050, groups=[1025, 1, 64, 3]),
    "long_1024": dict(n=2050, groups=[1024, 1, 64, 3]),
}

# gamma per (case family, regulariser): sized so that the prox zeroes between 5 % and 95 % of P (asserted on the restatements)
GAMMA = {
    "edges": {"l1": 1e-4, "sq_row": 1e-3, "sq_col": 3e-6, "ti": 3e-6, "l21": 1e-3, "squaredl21": 1e-5},
    "edges_gaps": {"l1": 3e-4, "sq_row": 1e-3, "sq_col": 3e-6, "ti": 3e-6, "l21": 1e-3, "squaredl21": 3e-5},  # at beta = 0
    "long": {"l1": 1e-4, "sq_row": 1e-3, "sq_col": 1e-6, "ti": 1e-6, "l21": 1e-4, "squaredl21": 1e-6},
}
PBCD_K = (3, 5, 32, 33, 64, 65)  # pb_grad: w = 4 with an idle lane, w = 8, two samples in flight, a partial block, a full one, two
# "edges" at degree 2 with k components: a row's norm grows with sqrt(k), and the row operators' thresholds with it
PBCD_K_GAMMA = {"l21": {3: 1e-3, 5: 1e-3, 32: 5e-3, 33: 5e-3, 64: 1e-2, 65: 1e-2},
                "squaredl21": {3: 1e-5, 5: 1e-5, 32: 3e-5, 33: 3e-5, 64: 1e-4, 65: 1e-4}}


def gamma_of(case, reg):
    return GAMMA["long" if case.startswith("long") else case][reg]


class Csr:
    def __init__(self, indptr, indices, data, n, d):
        self.indptr, self.indices, self.data, self.n, self.d = (np.asarray(indptr, np.int64), np.asarray(indices, np.int64),
                                                                np.asarray(data, np.float64), n, d)


def counts_of(group, n):
    """the column lengths of one group"""
    if isinstance(group, int):
        return [n // group + (1 if f < n % group else 0) for f in range(group)]
    assert sum(group) == n and min(group) >= 1, group
    return list(group)


def banded_one_hot(n, groups, gaps=False, pad=None, seed=0):
    """-> (Csr, ids): ids[g] the column ids of group g's features, ascending"""
    rng = np.random.default_rng(seed)
    pad = pad or [0] * len(groups)
    m = len(groups)
    indices = np.zeros((n, m), dtype=np.int64)
    ids, nxt = [], 0
    for g, group in enumerate(groups):
        counts = counts_of(group, n)
        cols = nxt + (2 if gaps else 1) * np.arange(len(counts))
        nxt = int(cols[-1]) + (2 if gaps else 1) + (pad[g] if gaps else 0)
        indices[rng.permutation(n), g] = np.repeat(cols, counts)
        ids.append(cols)
    data = rng.uniform(0.5, 1.5, (n, m)) * rng.choice([-1.0, 1.0], (n, m))
    return Csr(np.arange(n + 1) * m, indices.reshape(-1), data.reshape(-1), n, nxt), ids


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASES[name]
    Xo, ids = banded_one_hot(c["n"], c["groups"], c.get("gaps", False), c.get("pad"), seed=len(name))
    y = np.random.default_rng(31).standard_normal(Xo.n)
    for a in (Xo.indptr, Xo.indices, Xo.data, y):
        a.setflags(write=False)
    return Xo, y, ids


def inputs(name):
    """(Xo, y): shared between callers and read-only"""
    return _inputs(name)[:2]


def group_ids(name):
    return _inputs(name)[2]


def empty_columns(name):
    Xo = inputs(name)[0]
    used = np.zeros(Xo.d, dtype=bool)
    used[Xo.indices] = True
    return np.flatnonzero(~used)


def start(Xo, degree, k, fit_lower, fit_linear, fit_intercept, seed=1):
    """the start values of check_parity in the three GPU files: (P0, w0, b0, number of dummy features)"""
    P0, w0, b0, n_aug = init_fm(Xo.d, degree, k, fit_lower, fit_linear, seed=seed, scale=0.1)
    w0 = np.random.default_rng(seed + 5).uniform(-0.1, 0.1, Xo.d) if fit_linear else w0
    return P0, w0, (0.05 if fit_intercept else 0.0), n_aug


def launches(widths, wide_min):
    """what sweep_levels / sweep_runs issue for a sequence of level (run) widths: ("wide", width) per launch of its own,
    ("narrow", [widths]) per one-workgroup walk over consecutive narrower ones"""
    out = []
    for w in widths:
        if w >= wide_min:
            out.append(("wide", w))
        elif out and out[-1][0] == "narrow":
            out[-1][1].append(w)
        else:
            out.append(("narrow", [w]))
    return out
