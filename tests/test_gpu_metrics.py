"""-m gpu: nfm_score / nfm_metrics (metrics.hip) against oracle/metrics.py: the reference's own
known-answer tests (tests/test_metrics.nim:5-46) pushed through the device path, random scores with ties,
and `score` after a fit; sizes beyond one launch of the
group kernels, tie groups across hipcub tiles, zeros of both signs, infinities, and the smallest and most awkward n."""
import math

import numpy as np
import pytest

import nimfm_amd as nf
from oracle import metrics as M
from test_oracle_metrics import ROCAUC_KAT

pytestmark = pytest.mark.gpu


def model_with_scores(scores, task):
    """a linear-only model on the identity dataset: decisionFunction == scores exactly"""
    n = len(scores)
    X = nf.newCSRDataset(data=np.ones(n), indices=np.arange(n), indptr=np.arange(n + 1), nSamples=n, nFeatures=n)
    fm = nf.newFactorizationMachine(task, nComponents=1, warmStart=True)
    fm.set_params(np.zeros((1, 1, n)), np.asarray(scores, dtype=np.float64), 0.0)
    assert np.array_equal(fm.decisionFunction(X), np.asarray(scores, dtype=np.float64))
    return fm, X


def test_reference_known_answers_on_device():
    for yt, ys, want in ROCAUC_KAT:
        fm, X = model_with_scores(ys, "classification")
        # rocauc's positive class is yTrue == 1; the device path sees targets through sgn (pos <-> y > 0)
        got = fm.metrics(X, [1.0 if v == 1 else -1.0 for v in yt])["rocauc"]
        assert got == want, (yt, ys, got)
    fm, X = model_with_scores([-0.1, 0.1, 0.9, -0.2], "classification")
    assert fm.score(X, [-1.0, -1.0, 1.0, 1.0]) == 0.5  # accuracy(yTrue, sgn(yScore2)), test_metrics.nim:41


@pytest.mark.parametrize("n,ties", [(1000, False), (50_000, True), (300_001, True)])
def test_random_scores(n, ties):
    rng = np.random.default_rng(n)
    s = rng.standard_normal(n)
    if ties:
        s = np.round(s, 2)  # many equal scores: the trapezoid groups
    y = np.sign(s + rng.standard_normal(n))
    y[y == 0] = 1.0
    fm, X = model_with_scores(s, "classification")
    got = fm.metrics(X, y)
    assert got["accuracy"] == M.accuracy(np.sign(y).astype(np.int64), np.sign(s).astype(np.int64))
    assert got["rocauc"] == M.rocauc(y.astype(np.int64), s)  # integer trapezoid sums: bit for bit
    assert abs(got["rmse"] - M.rmse(y, s)) <= 1e-11 * M.rmse(y, s)  # the reference adds left to right, the device by a tree
    assert fm.score(X, y) == got["accuracy"]
    fm.task = "regression"
    fm2, _ = model_with_scores(s, "regression")
    assert abs(fm2.score(X, y) - M.rmse(y, s)) <= 1e-11 * M.rmse(y, s)  # the reference adds left to right, the device by a tree
    assert fm2.metrics(X, y) == fm2.metrics(X, y)  # reproducible


def against_oracle(s, y, rocauc=None):
    """rocauc and accuracy bit for bit; rmse within n * 2^-53 relative of the correctly rounded sum of the same squares:
    any order of adding n non-negative doubles is within (n - 1) * 2^-53 of their exact sum, relative, and the square
    root halves that -- a derived bound, far below what one dropped partial sum of a tree changes."""
    s, y = np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(s)
    fm, X = model_with_scores(s, "classification")
    got = fm.metrics(X, y)
    want_auc = M.rocauc(y.astype(np.int64).tolist(), s.tolist()) if rocauc is None else rocauc
    want_acc = M.accuracy(np.sign(y).astype(np.int64).tolist(), np.sign(s).astype(np.int64).tolist())
    assert got["rocauc"] == want_auc or (np.isnan(got["rocauc"]) and np.isnan(want_auc)), (n, got, want_auc)
    assert got["accuracy"] == want_acc == fm.score(X, y), (n, got, want_acc)
    want_rmse = math.sqrt(math.fsum((s - y) ** 2) / n)
    if math.isinf(want_rmse):
        assert got["rmse"] == want_rmse
    else:
        assert abs(got["rmse"] - want_rmse) <= n * 2.0 ** -53 * want_rmse, (n, got["rmse"], want_rmse)
    fm2, _ = model_with_scores(s, "regression")
    assert fm2.score(X, y) == got["rmse"]
    return got


N_BEYOND = 1_100_000  # k_auc_groups, k_group_heads and k_pos_flags launch at most 4096 x 256 = 1 048 576 threads


@pytest.mark.parametrize("distinct", [7, 1])
def test_beyond_one_pass_of_the_group_kernels(distinct):
    """n above one launch; 7 distinct scores: tie groups of about 157 000, across workgroups, grid passes and hipcub tiles.
    All scores equal: one group, rocauc exactly 0.5."""
    rng = np.random.default_rng(distinct)
    s = np.array([-2.5, -1.0, -0.125, 0.25, 0.5, 1.75, 3.0])[rng.integers(0, distinct, size=N_BEYOND)]
    y = np.sign(s + 2.0 * rng.standard_normal(N_BEYOND))
    y[y == 0] = 1.0
    assert N_BEYOND > 4096 * 256 and len(np.unique(s)) == distinct and len(np.unique(y)) == 2
    got = against_oracle(s, y)
    if distinct == 1:
        assert got["rocauc"] == 0.5


def test_zeros_and_infinities():
    """Scores of +0.0 and -0.0 are one tie group whatever their labels, +inf and -inf sort to the ends; a target of 0.0 is
    not a positive for rocauc and a sign match only for a score of 0.  (decisionFunction adds a sample's terms to +0.0, so
    a -0.0 weight arrives at the metrics as +0.0: the case pins what the public call gives for such scores.)"""
    s = np.array([0.0, -0.0, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, np.inf, -np.inf, -0.0, 0.0, 0.5, -0.5])
    y = np.array([1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0, 1.0, 1.0])
    got = against_oracle(s, y)
    assert math.isinf(got["rmse"])
    # the four labelled zeros alone: one group of two positives and two negatives between one positive and one negative
    got = against_oracle([1.0, 0.0, -0.0, -0.0, 0.0, -1.0], [1.0, 1.0, -1.0, 1.0, -1.0, -1.0], rocauc=(2 * (1 + 3) / 2 + 1 * (3 + 3) / 2) / 9.0)
    rng = np.random.default_rng(8)
    n = 70_001
    s = np.array([-np.inf, -1.5, -0.0, 0.0, 0.5, np.inf])[rng.integers(0, 6, size=n)]
    y = np.array([-1.0, 0.0, 1.0])[rng.integers(0, 3, size=n)]
    against_oracle(s, y)


@pytest.mark.parametrize("n", [1, 2, 257, 262_145])
def test_tiny_and_awkward_sizes(n):
    """one and two samples, one past a workgroup, and one past 1024 x 256, where k_sqerr_partial's slice per workgroup
    becomes 2 and the last workgroups get empty slices"""
    rng = np.random.default_rng(n)
    s = np.round(rng.standard_normal(n), 1)
    y = np.sign(s + rng.standard_normal(n))
    y[y == 0] = 1.0
    if n == 2:
        y = np.array([1.0, -1.0])  # both classes
    against_oracle(s, y)


def test_degenerate_and_errors():
    fm, X = model_with_scores([0.3, 0.2, 0.1], "classification")
    assert np.isnan(fm.metrics(X, [1.0, 1.0, 1.0])["rocauc"])  # one class only: 0/0 as in the reference
    fm = nf.newFactorizationMachine("regression", nComponents=2)
    with pytest.raises(nf.NotFittedError):
        fm.score(X, [0.0, 0.0, 0.0])
