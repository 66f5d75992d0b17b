"""Plain-Python restatement of OmegaCS's BCD hooks (regularizer/omegacs.nim:31-85: initBCD, computeCacheBCD with its
recompute, prox, updateCacheBCD) and of its eval (:15-28), run inside tests/pbcd_restatement.py's `fit`: that loop is the
reference's pbcd.nim at maxSearch = 0 and knows its regulariser through four hooks only.  `fit` below puts an OmegaCS hook
object in the place of pbcd_restatement.Reg for the length of one call.

OmegaCS keeps the degree-0..deg ANOVA polynomials of every row's norm in `cache` and the ones without the current row in
`dcache`.  initBCD sizes both by the MODEL's degree and is the only place that writes dcache as a whole: dcache persists
across features, orders and iterations of one fit.  computeCacheBCD takes deg = degree - order; `fit` does not hand the hook
a degree, so the hook counts its calls modulo nOrders.

`last_prox_recomputes` / `last_update_recomputes` count the two exact-recompute branches (omegacs.nim:71-79, :60-61) taken in
the last fit.  `Slow` is the brute-force prox of tests/regularizer/omegacs_slow.nim:28-45: nothing cached, the threshold is
lam times the degree-(deg - 1) ANOVA polynomial of all current norms but row j's.
"""
import math

import pbcd_restatement as B
from pbcd_restatement import norm2

last_prox_recomputes = 0
last_update_recomputes = 0


def anova_of_norms(norms, deg):
    """the ANOVA polynomials of degree 0 .. deg of `norms` by recomputeCacheBCD's recursion (omegacs.nim:40-44): j outer, the
    degree descending inside it -> cache[0 .. deg]"""
    cache = [0.0] * (deg + 1)
    cache[0] = 1.0
    for nj in norms:
        for g in range(deg):
            cache[deg - g] += cache[deg - g - 1] * nj
    return cache


def eval_omegacs(Po, deg):
    """Po [d + nAug][k] -> the degree-deg ANOVA polynomial of the row norms"""
    return anova_of_norms([norm2(r) for r in Po], deg)[deg]


class OmegaCS:
    """the hooks `fit` calls, with pbcd_restatement.Reg's interface"""
    name = "omegacs"
    chained = True

    def __init__(self, degree, nFeatures, nOrders, transpose=False):
        if transpose:
            raise ValueError("OmegaCS has no transpose.")
        self.degree, self.nOrders = degree, nOrders
        self.calls = 0
        self.deg = degree
        self.prox_recomputes = self.update_recomputes = 0
        self.resums = 0
        self.norms = [0.0] * nFeatures  # initBCD
        self.cache = [0.0] * (degree + 1)
        self.dcache = [0.0] * (degree + 1)
        self.dcache[1] = 1.0
        self.value = 0.0

    def recompute(self, deg):
        for t in range(len(self.cache)):
            self.cache[t] = 0.0
        self.cache[0] = 1.0
        for nj in self.norms:
            for g in range(deg):
                self.cache[deg - g] += self.cache[deg - g - 1] * nj
        self.value = self.cache[deg]

    def compute_cache(self, Po):
        self.deg = self.degree - self.calls % self.nOrders
        self.calls += 1
        for j in range(len(Po)):
            self.norms[j] = norm2(Po[j])
        self.recompute(self.deg)

    def prox(self, pj, lam, j):
        deg, cache, dcache = self.deg, self.cache, self.dcache
        nrm = norm2(pj)
        for g in range(2, deg + 1):
            dcache[g] = cache[g - 1] - dcache[g - 1] * self.norms[j]
        if min(dcache) < 0:
            self.prox_recomputes += 1
            self.norms[j] = 0.0
            self.recompute(deg - 1)
            dcache[0] = 0.0
            dcache[1] = 1.0
            for g in range(2, deg + 1):
                dcache[g] = cache[g - 1]
            self.norms[j] = nrm
            self.recompute(deg)
        if nrm > lam * dcache[deg]:
            f = 1.0 - lam * dcache[deg] / nrm
            for s in range(len(pj)):
                pj[s] *= f
        else:
            for s in range(len(pj)):
                pj[s] = 0.0

    def update_cache(self, pj, j):
        deg, cache, dcache = self.deg, self.cache, self.dcache
        nn = norm2(pj)
        for g in range(1, deg + 1):
            cache[g] += dcache[g] * nn
            cache[g] -= dcache[g] * self.norms[j]
        self.norms[j] = nn
        if min(cache) < 0:
            self.update_recomputes += 1
            self.recompute(deg)
        self.value = cache[deg]


class Slow(OmegaCS):
    """omegacs_slow.nim:28-45: every threshold from all the current norms, nothing carried from step to step"""

    def compute_cache(self, Po):
        self.deg = self.degree - self.calls % self.nOrders
        self.calls += 1
        self.Po = Po

    def prox(self, pj, lam, j):
        norms = [math.sqrt(sum(x * x for x in r)) for r in self.Po]  # row j of Po IS pj: `fit` steps it in place
        nrm = norms[j]
        norms[j] = 0.0
        strength = lam * anova_of_norms(norms, self.deg - 1)[self.deg - 1]
        shrink = 1.0 - strength / nrm if nrm > strength else 0.0
        for s in range(len(pj)):
            pj[s] *= shrink

    def update_cache(self, pj, j):
        pass


def fit(indptr, indices, data, y, P, w, intercept, degree, nAugments, fitLinear, fitIntercept, slow=False, transpose=False,
        **kw):
    """pbcd_restatement.fit with OmegaCS (or its brute-force twin) as the regulariser; every other argument is its own"""
    global last_prox_recomputes, last_update_recomputes
    nOrders = len(P)
    made = []

    def factory(name, transpose_, degree_, nFeatures):
        made.append((Slow if slow else OmegaCS)(degree_, nFeatures, nOrders, transpose_))
        return made[-1]

    saved = B.Reg
    B.Reg = factory
    try:
        out = B.fit(indptr, indices, data, y, P, w, intercept, degree, nAugments, fitLinear, fitIntercept, reg="omegacs",
                    transpose=transpose, **kw)
    finally:
        B.Reg = saved
    last_prox_recomputes, last_update_recomputes = made[0].prox_recomputes, made[0].update_recomputes
    return out
