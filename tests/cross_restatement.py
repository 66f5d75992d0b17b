"""crossDecisionFunction and recommend restated in plain Python; independent of oracle/ and of the library.

A row is a list of (column id, value) in storage order: it may be empty, unsorted, or repeat an id.  P is [k][d + nAug] (the
one order of a degree-2 model), w [d], lams [k]; nAug is 0 or 1 (model/factorization_machine.nim:81-86 at degree 2).

    joined_row     tensor/sparse.nim:671-698: row i of hstack(U[rep], V[tile]) -- u, then v with its ids moved up by U's width
    joined_score   model/factorization_machine.nim:100-122 on that row: linear (kernels.nim:14-19), the intercept, the dummy
                   feature appended once (:112), then per factor anova of degree 2 (kernels.nim:59-64) times lams[s] (:120)
    factored_score the same number from one pass per side and one product over the factors
    rank           recommend's order: descending score, then ascending id; NaN below every number
"""
import math


def joined_row(u, v, dU):
    return list(u) + [(j + dU, x) for j, x in v]


def _sums(row, Ps):
    """kernels.nim:59-64: q = sum_j P[s,j] x_j and r = sum_j (P[s,j] x_j)^2, in storage order"""
    q = r = 0.0
    for j, x in row:
        t = Ps[j] * x
        q += t
        r += t * t
    return q, r


def _linear(row, w, col0=0):
    acc = 0.0
    for j, x in row:  # kernels.nim:14-19
        acc += w[j + col0] * x
    return acc


def joined_score(u, v, dU, dV, P, w, b, lams, nAug):
    row = joined_row(u, v, dU)
    out = _linear(row, w) + b  # factorization_machine.nim:108-110 (the dummy feature is not there yet)
    row = row + [(dU + dV + t, 1.0) for t in range(nAug)]  # :112, dataset.nim:182-189
    for s in range(len(P)):  # :116-120
        q, r = _sums(row, P[s])
        out += lams[s] * ((q * q - r) / 2.0)
    return out


def side(row, col0, P, w, lams, extra=()):
    """-> (q [k], the side's own scalar lin + 1/2 sum_s lams[s] (q_s^2 - r_s)); extra: entries in the model's own columns
    (the dummy feature, which joins the U side)"""
    ent = [(j + col0, x) for j, x in row] + list(extra)
    qs, own = [], 0.0
    for s in range(len(P)):
        q, r = _sums(ent, P[s])
        qs.append(q)
        own += lams[s] * ((q * q - r) / 2.0)
    return qs, _linear(row, w, col0) + own


def factored_score(u, v, dU, dV, P, w, b, lams, nAug):
    qu, au = side(u, 0, P, w, lams, extra=[(dU + dV + t, 1.0) for t in range(nAug)])
    qv, cv = side(v, dU, P, w, lams)
    dot = 0.0
    for s in range(len(P)):
        dot += (lams[s] * qu[s]) * qv[s]
    return ((b + au) + cv) + dot


def cross(case, score=joined_score):
    P, w, lams = [list(map(float, r)) for r in case["P"]], list(map(float, case["w"])), list(map(float, case["lams"]))
    return [[score(u, v, case["dU"], case["dV"], P, w, float(case["b"]), lams, case["nAug"]) for v in case["V"]] for u in case["U"]]


def rank_key(j, s):
    """sorts ascending into recommend's order"""
    return (1, 0.0, j) if math.isnan(s) else (0, -s, j)


def rank(scores_row, K):
    """-> the K pairs (j, score)"""
    order = sorted(range(len(scores_row)), key=lambda j: rank_key(j, scores_row[j]))
    return [(j, scores_row[j]) for j in order[:K]]
