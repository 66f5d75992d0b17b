"""The restatement of crossDecisionFunction / recommend against itself (tests/cross_restatement.py, no GPU): the factored form
the kernels compute against the joined-row definition, and the cases' margins, which make recommend's ids decidable."""
import math
import struct

import pytest

import cross_restatement as R
from cross_cases import cases

CASES = cases()
# decisionFunction against an independently ordered recursion: tests/test_gpu_psgd_lazy.py:245, smoke()'s bound for the exact order
RTOL, ATOL = 1e-9, 1e-12
MIN_GAP = 1e-6  # relative, between neighbouring scores among ranks 1 .. K + 1


def bits(x):
    return struct.pack("<d", x)


@pytest.fixture(scope="module")
def scored():
    return {c["name"]: (R.cross(c, R.joined_score), R.cross(c, R.factored_score)) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_factored_form_is_the_joined_row_form(case, scored):
    joined, factored = scored[case["name"]]
    worst = 0.0
    for ju, fu in zip(joined, factored):
        for a, b in zip(ju, fu):
            worst = max(worst, abs(a - b) / (ATOL + RTOL * abs(a)))
            assert abs(a - b) <= ATOL + RTOL * abs(a), (a, b)
    print("%s: worst |factored - joined| / bound = %.3g" % (case["name"], worst))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_margins_make_the_ranking_decidable(case, scored):
    joined, _ = scored[case["name"]]
    K, tie = case["K"], case["tie"]
    for row in joined:
        top = R.rank(row, min(K + 1, len(row)))
        for (j0, s0), (j1, s1) in zip(top, top[1:]):
            if tie and {j0, j1} == set(tie):
                continue
            assert s0 - s1 >= MIN_GAP * max(abs(s0), abs(s1)), (case["name"], j0, j1, s0, s1)


def test_planted_tie_has_identical_bits():
    case = next(c for c in CASES if c["tie"])
    a, b = case["tie"]
    in_top = 0
    for score in (R.joined_score, R.factored_score):
        for row in R.cross(case, score):
            assert bits(row[a]) == bits(row[b])
            top = [j for j, _ in R.rank(row, case["K"])]
            if a in top and b in top:
                assert top.index(a) + 1 == top.index(b)  # neighbours, the smaller id first
                in_top += 1
    assert in_top > 0  # the tie is inside some user's top K: recommend has to resolve it


def test_ranking_rule():
    nan = float("nan")
    row = [1.0, nan, 3.0, 3.0, -math.inf, nan, 0.0, -0.0, math.inf]
    assert [j for j, _ in R.rank(row, len(row))] == [8, 2, 3, 0, 6, 7, 4, 1, 5]


def test_the_dummy_feature_joins_the_user_side():
    case = next(c for c in CASES if c["nAug"] == 1)
    u, v = case["U"][2], case["V"][3]
    P, w, lams = [list(r) for r in case["P"]], list(case["w"]), list(case["lams"])
    d = case["dU"] + case["dV"]
    qu, _ = R.side(u, 0, P, w, lams, extra=[(d, 1.0)])
    qu0, _ = R.side(u, 0, P, w, lams)
    assert all(abs((a - b) - P[s][d]) <= 1e-15 * (1 + abs(a)) for s, (a, b) in enumerate(zip(qu, qu0)))
    assert any(P[s][d] != 0.0 for s in range(case["k"]))
