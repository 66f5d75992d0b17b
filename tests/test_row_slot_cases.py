"""CPU: the conditions the inputs of tests/row_slot_cases.py must meet so that tests/test_gpu_row_slots.py runs the row phase
and decisionFunction on every lane mapping (L, SPLIT) and on every kernel the host can choose there.  No GPU: the restatement
of the host's choice only, and the strings of the sources it restates where no program runs them (the row phase's choice is
run: tests/test_cpp_mb_route.py).

Coverage is asserted, not claimed: every conceivable (MODE, singles, GEN) per lane mapping and solver is either reached by a
case of the table or ruled out by name in why_unreachable(), and the test fails on anything that is neither.  Run with -s to see
the 24 pairs and what reaches them."""
import os

import numpy as np
import pytest

import row_slot_cases as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_source_still_has_the_choices_restated():
    """the strings of the sources the restatement follows that no program checks: choose_split, the kernels' own constants, and
    the choices of api.hip, plan.hip and predict.hip.  The row phase's choice itself (slots, mode, the two-wavefront kernel, the
    stored batch, the staged weights) is csrc/mb_route.h's, which tests/test_cpp_mb_route.py runs against the restatement."""
    kern, api, pred, mb, plan = (src(f) for f in ("mb_fm_kernels.h", "api.hip", "predict.hip", "mb_fm.hip", "plan.hip"))
    common = src("common.h") + src("lane_map.h")  # common.h includes lane_map.h: choose_split, for g++ as well
    assert '#include "lane_map.h"' in src("common.h")
    assert "constexpr int kWave = 64;" in common
    assert 'if (const char* env = getenv("NFM_SPLIT")) {' in common  # inside choose_split: read per call
    assert "if (s >= 1) return s > R ? R : (s > 16 ? 16 : p2(s));" in common
    assert "while (r < v && r < 64) r <<= 1;" in common
    assert "constexpr int CAP = E * LPS;" in kern
    assert "constexpr bool CAN_REG = CAN_HOLD && !GEN && OPT == OPT_SGD && L * SPLIT == kWave;" in kern
    assert "wq[e] = a.Wt[(size_t)pib * CAP + q];" in kern
    assert "m->cfg.degree == 2 && m->nb == 1 && (o->batch == 1 || lambda <= 1.4);" in api
    assert "const bool gen = !(M.nb == 1 && M.degree == 2);" in mb
    # (the boundaries are plan_route.h's plan_bounds, which tests/test_cpp_plan_route.py runs)
    assert "if (first_singleton && ns > 0) { pos = 1; B.bat_pos.push_back(1); }" in src("plan_route.h") and "= plan_bounds(ns, " in plan
    assert "if (!on || M.kind != NFM_KIND_FM || M.nb < 2 || M.kc != 1 || M.bs != M.da || M.rs != 1) return NFM_OK;" in pred
    assert "if (LT > kWave || X.nnz + (int64_t)M.n_aug * X.n < 2 * M.da) return NFM_OK;" in pred
    assert 'if (R >= 2 && split < 2 && !getenv("NFM_SPLIT")) split = 2;' in pred
    assert "if constexpr (R >= 8) if (split >= 8) return launch_fm_predict_orders<LT, 8>(ctx, X, M, Pf, lgL, out);" in pred
    assert "if (R >= 16 && split >= 16) return launch_fm_predict<L, (R >= 16 ? 16 : R)>(ctx, X, M, out);" in pred


def test_slot_counts():
    assert [R.lanes_for_k(k) for k in R.KS] == [1, 2, 4, 8, 16, 32]
    assert all(k < 2 * R.lanes_for_k(k) for k in R.KS)  # padding lanes or a padding component
    assert len(R.PAIRS) == 24
    for L in (1, 2, 4, 8, 16, 32):
        top = min(64 // L, 16)
        for q in range(1, 70):
            assert R.row_slots(L, q) == min(R.p2(q), top), (L, q)
        reqs = R.requests(L)
        assert reqs[:-1] == [s for s in (1, 2, 4, 8, 16) if s <= top] and reqs[-1] == (16 if 64 // L < 16 else 64)
        assert reqs[-1] > top and R.row_slots(L, reqs[-1]) == top  # the clamping request
    assert [R.held_entries(L, s) for L, s in ((1, 4), (1, 8), (8, 1), (8, 2), (4, 4), (16, 2), (32, 1), (32, 2), (8, 8))] == [0, 4, 4, 4, 4, 2, 2, 1, 1]
    assert {R.held_capacity(L, s) for L, s in R.PAIRS} == {0, 32, 64}
    assert all(R.held_capacity(L, s) == (0 if L * s < 8 else 32 if L * s == 8 else 64) for L, s in R.PAIRS)


# ---------------------------------------------------------------- (b) the data
@pytest.mark.parametrize("family", ["short", "long"])
@pytest.mark.parametrize("regime", ["dense", "sparse"])
def test_datasets_have_the_stated_lengths(family, regime):
    X, y = R.train_data(family, regime)
    d, batch = R.REGIMES[regime]
    lens = R.FAMILIES[family]
    assert X.n == R.N_TRAIN == len(y) and X.d == d
    assert X.lengths().tolist() == [lens[(i - 1) % len(lens)] for i in range(X.n)]
    assert max(lens) == (32 if family == "short" else 150)
    unsorted = 0
    for i in range(X.n):
        row = X.indices[X.indptr[i]:X.indptr[i + 1]]
        assert len(np.unique(row)) == len(row) and (len(row) == 0 or (row.min() >= 0 and row.max() < d))
        if i % 2 == 0:
            assert np.all(np.diff(row) > 0)
        elif len(row) >= 2:
            assert not np.all(np.diff(row) > 0)
            unsorted += 1
    assert unsorted > X.n // 3
    assert np.abs(X.data).max() < 1.0
    # each of the edge lengths of the family in the first and in the last mini-batch of both epochs, for SGD (301, 301, 98) and
    # for AdaGrad, whose first epoch opens with a batch of one sample: there the first FULL batch is meant
    perms = R.train_perms(family, regime)
    edges = [m for m in R.EDGE_LENGTHS if m in lens]
    assert edges == ([31, 32] if family == "short" else [31, 32, 33, 64, 65])
    for e in range(2):
        order = np.arange(X.n) if perms is None else perms[e]
        assert sorted(order.tolist()) == list(range(X.n))
        for first in (False, True) if e == 0 else (False,):
            cuts = R.batches(X.n, batch, first)
            assert cuts[0][0] == 0 and cuts[-1][1] == X.n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            sizes = [hi - lo for lo, hi in cuts]
            if regime == "dense":
                assert sizes == ([1, 301, 301, 97] if first else [301, 301, 98])
                assert all(s % 4 for s in sizes if s > 1)  # every samples-per-block count from 4 to 256 ends inside a block
            else:
                assert sizes == ([1] + [129] * 5 + [54] if first else [129] * 5 + [55])
            for lo, hi in (cuts[1 if first else 0], cuts[-1]):
                have = set(X.lengths()[order[lo:hi]].tolist())
                assert set(edges) <= have, (family, regime, e, first, lo, hi, sorted(set(edges) - have))
    first = int(X.lengths()[0 if perms is None else perms[0][0]])
    assert first == (max(lens) if perms is None else 2)  # the sample of AdaGrad's stored first batch: lengths_csr, train_perms
    if regime == "sparse":  # the popular ids: two per row of two entries or more, none elsewhere
        hub = X.indices < R.N_HUBS
        per_row = np.add.reduceat(hub.astype(np.int64), X.indptr[:-1][X.lengths() > 0])
        assert per_row.tolist() == [2 if m >= 2 else 0 for m in X.lengths() if m > 0]
    else:
        assert d == 200


def test_predict_dataset():
    X = R.predict_data()
    assert X.n == R.N_PREDICT == 261 and X.d == 200 and X.n % 4 == 1
    assert X.lengths().tolist() == [R.LONG[(i - 1) % len(R.LONG)] for i in range(X.n)]
    assert len(X.data) >= 2 * (X.d + 2)  # nnz >= 2 * da: predict_orders takes the calls it can


# ---------------------------------------------------------------- (c) the regimes
@pytest.mark.parametrize("group", R.groups(), ids=lambda g: "-".join(str(v) for v in g))
def test_regimes_are_what_they_claim(group):
    k, family, regime, solver, model = group
    X, _ = R.train_data(family, regime)
    d, batch = R.REGIMES[regime]
    degree, fit_lower, fit_linear = R.MODELS[model]
    lam = batch * (len(X.data) / X.n) / d
    singles = R.use_singles(solver, degree, R.n_orders(degree, fit_lower), batch, len(X.data), X.n, d)
    if regime == "dense":
        assert lam > 1.4 and not singles
    else:
        assert lam <= 1.4 and singles == (degree == 2)
        assert model in ("deg2", "deg2_aug")
    paths = [p for c in R.cases_of(group) for p in R.fit_paths(c)]
    assert all(p.singles == singles for p in paths)
    if model == "deg2_aug":  # the dummy feature takes the widest row from 150 to 151 entries, and rows of 32 and 64 past a chunk
        assert R.n_augments(degree, fit_lower, fit_linear) == 1 and max(p.widest for p in paths) == 151


# ---------------------------------------------------------------- (a) coverage of the row phase
def why_unreachable(L, s, solver, gen, mode, singles):
    """None, or the reason why no input makes the host launch k_row_phase<L, s, .., gen, mode, ..> for a batch with (without)
    singles; environment knobs that are read once per process (NFM_HELD, NFM_NQ, NFM_ADA2) stay at their defaults"""
    lps, held = L * s, R.held_entries(L, s) > 0
    if singles and gen:
        return "singles need one order of degree 2 (api.hip:1769)"
    if mode and not held:
        return "no held entries below 8 lanes per sample (held_entries)"
    if mode == 0 and held and not gen:
        return "a held lane mapping streams only models without an interaction block, and those are GEN (mode_for)"
    if mode == 0 and held and singles:
        return "degree 1 has no singles (api.hip:1769)"
    if mode == 2 and not (solver == "sgd" and not gen and lps == 64 and singles):
        return "MODE 2 / 4 is SGD with singles, one order of degree 2, one sample per wavefront (mode_for)"
    if mode == 1 and solver == "sgd" and not gen and lps == 64 and singles:
        return "SGD with singles at L * SPLIT = 64 takes MODE 2 (mode_for)"
    if mode == 1 and solver == "adagrad" and L == 32 and singles:
        return ("k_row_phase_ada2 takes every AdaGrad batch with singles and rows of at most 64 entries at L = 32 but the stored first "
                "one, a single sample; longer rows are MODE 3")
    return None


GEN_LS = tuple(R.lanes_for_k(k) for k in R.GEN_KS)


def reached():
    out, ada2 = {}, set()
    for c in R.table():
        for p in R.fit_paths(c):
            if p.samples == 1 and p.stored:  # AdaGrad's first step, a single sample: not what reaches a kernel here
                continue
            if p.kernel == "ada2":
                ada2.add((c.request, c.solver))
                continue
            solver = "adagrad" if c.solver == "mbpsgd" else c.solver  # MBPSGD's row phase is AdaGrad's reading the stored parameters
            out.setdefault((p.L, p.slots, solver, p.gen, p.mode, p.singles), set()).add((c.model, c.family, c.regime, c.solver))
            assert p.sing == (p.mode == 0 and p.singles and not p.gen)
            assert (p.held, p.cap) == (R.held_entries(p.L, p.slots), R.held_capacity(p.L, p.slots))
    return out, ada2


def test_the_table_reaches_every_kernel_of_every_lane_mapping():
    got, ada2 = reached()
    seen_pairs = {(L, s) for (L, s, *_rest) in got}
    assert seen_pairs == set(R.PAIRS)
    missing, excluded = [], {}
    for L, s in R.PAIRS:
        line = []
        for solver in ("sgd", "adagrad"):
            for gen in (False, True):
                for mode in (0, 1, 2, 3):
                    for singles in (False, True):
                        key = (L, s, solver, gen, mode, singles)
                        why = why_unreachable(*key)
                        # GEN with an interaction block is in the table at k = 7 and k = 13 only; degree 1 (MODE 0) at every k
                        optional = gen and mode != 0 and L not in GEN_LS
                        if why is not None:
                            assert key not in got, (key, why)
                            excluded.setdefault(why, 0)
                            excluded[why] += 1
                        elif key in got:
                            line.append("%s%s M%d%s%s" % (solver[0], "G" if gen else "", mode, "+sing" if singles else "",
                                                          "(SING)" if mode == 0 and singles else ""))
                        elif not optional:
                            missing.append(key)
        print("L %2d SPLIT %2d  E %d CAP %2d | %s" % (L, s, R.held_entries(L, s), R.held_capacity(L, s), ", ".join(line)))
    for why, cnt in sorted(excluded.items()):
        print("never chosen (%3d combinations): %s" % (cnt, why))
    assert not missing, missing
    # the two-wavefront AdaGrad route ignores the request: every request at L = 32 ends there
    assert ada2 == {(q, "adagrad") for q in R.requests(32)}
    # what the issue names: the streamed kernel with singles on all six mappings below 8 lanes, for both solvers
    sing = {(L, s) for (L, s, solver, gen, mode, singles) in got if mode == 0 and singles}
    assert sing == {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (4, 1)}
    # more than one held entry per lane, MODE 3 at CAP = 32, MODE 1 with singles below 64 lanes
    for solver in ("sgd", "adagrad"):
        for L, s in R.PAIRS:
            if R.held_entries(L, s) > 1:
                for mode, singles in ((1, False), (3, False), (3, True)) + (((1, True),) if not (solver == "adagrad" and L == 32) else ()):
                    assert (L, s, solver, False, mode, singles) in got
    assert all((8, 1, solver, gen, 3, False) in got for solver in ("sgd", "adagrad") for gen in (False, True))


def test_requests_that_clamp_share_a_signature_and_others_do_not():
    for g in R.groups():
        cases = R.cases_of(g)
        L = R.lanes_for_k(g[0])
        sigs = [R.signature(c) for c in cases]
        assert sigs[-1] == sigs[-2]  # the clamping request and the largest count
        ada2 = g[3] == "adagrad" and L == 32 and g[2] == "sparse" and g[1] == "short"
        if ada2:  # every batch but the first on k_row_phase_ada2, and the first is one row of two entries
            assert len(set(sigs)) == 1
            paths = R.fit_paths(cases[0])
            assert [p.kernel for p in paths].count("row") == 1 and paths[0].kernel == "row" and paths[0].widest == 2 and paths[0].samples == 1
        else:
            assert len(set(sigs)) == len(cases) - 1


def test_stage_w_case():
    """the k_stage_w table at a stride of 32: SGD, k = 13, short rows, one and two slots"""
    caps = {q: R.stage_w_cap(R.Case(13, q, "short", "dense", "sgd", "deg2")) for q in (1, 2, 4, 8)}
    assert caps == {1: 32, 2: 64, 4: 64, 8: 64}
    assert R.stage_w_cap(R.Case(13, 1, "long", "dense", "sgd", "deg2")) == 0  # MODE 3 is not staged


# ---------------------------------------------------------------- decisionFunction
def test_predict_reaches_every_lane_mapping_of_both_kernels():
    got = {}
    for model in R.PREDICT_MODELS:
        for k in R.KS:
            for q in R.requests(R.lanes_for_k(k)):
                got.setdefault(R.predict_kernel(k, q, model), set()).add(model)
    for model in ("deg2", "deg3_none", "deg3_augment"):  # one order: k_fm_predict on all 24 mappings, anova_fwd_degn at degree 3
        assert {(L, s) for (kind, L, s), ms in got.items() if kind == "predict" and model in ms} == set(R.PAIRS)
    orders = sorted((LT, s) for (kind, LT, s) in got if kind == "orders")
    assert orders == [(LT, s) for LT in (2, 4, 8, 16, 32, 64) for s in (1, 2, 4, 8) if s <= 64 // LT]
    for key in sorted(got):
        print("%-7s L/LT %2d SPLIT %2d | %s" % (key + (", ".join(sorted(got[key])),)))
    # three orders and a padding block at L = 32 are 128 lanes: no orders kernel, k_fm_predict walks the orders
    assert R.predict_kernel(50, 2, "deg4_explicit") == ("predict", 32, 2)
    assert R.predict_kernel(30, 2, "deg4_explicit") == ("orders", 64, 1)  # one slot whatever the request
    assert R.predict_kernel(7, 16, "deg3_explicit") == ("orders", 8, 8)  # k_fm_predict_orders has no 16-slot instance
    assert R.predict_kernel(13, 1, "deg3_explicit") == ("orders", 16, 1)  # <LT, 1> below LT = 64: never taken without NFM_SPLIT
