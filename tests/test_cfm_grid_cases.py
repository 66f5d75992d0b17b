"""CPU: the conditions the inputs of tests/cfm_grid_cases.py must meet so that the tests built on them
(tests/test_gpu_cfm_grid.py) reach the code they are there for and may keep the tolerances of tests/test_gpu_hazan.py and
tests/test_gpu_gcd.py.  No GPU: the restatements only.

Coverage is asserted, not claimed: kG, kBlock, kNarrowBlock, kHazanChunk and kCgMaxIter are read out of the sources, and the
number of partials and of fin_sum trips of every caller is recomputed from them per input, so a later retune of a constant
fails here instead of silently ending the coverage.

Distance of the restatements between the device's trees and in-order sums at forced counts, measured here.  Hazan, relative,
the maximum over P, lams, w and every loss: tall 1.8e-14, 3.4e-14 and 4.0e-14; broad 7.4e-15, 1.0e-15 and 1.1e-14; long 2.4e-12
and 8.8e-14; edges_n at most 3.4e-14; edges_d at most 1.9e-14; cg_long 1.1e-12; the power-edge grid cases at most 1e-13.  All
are below the 1e-8 of tests/test_hazan_restatement.py.  GreedyCD, as the largest fraction of a tolerance of the device
comparison: tall 1.0e-6, 5.2e-7 and (logistic) 7.9e-6, long 7.8e-6, broad 2.5e-7: below the 1e-2 of
tests/test_gcd_restatement.py.  No tolerance is widened.  `cg_cap` is compared with nothing but its CG count: there the two
summations end 6.3e-5 apart on w after 1000 CG iterations, and its test holds only that both are still 10x above the CG's
tolerance then."""
import functools
import os
import re

import numpy as np
import pytest

import cfm_grid_cases as G
import gcd_cases as gc
import gcd_restatement as gr
import hazan_restatement as hr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")


def _const(name, file):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


kBlock, kNarrowBlock, kG = _const("kBlock", "common.h"), _const("kNarrowBlock", "cd_dev.h"), _const("kG", "cfm_dev.h")
kHazanChunk, kCgMaxIter = _const("kHazanChunk", "cfm.h"), _const("kCgMaxIter", "cfm.h")
kGroups = kBlock // kG


def ceil_div(a, b):
    return -(-a // b)


def test_the_source_still_has_the_loops_these_numbers_describe():
    dev, cfm, gcd = (open(os.path.join(CSRC, f)).read() for f in ("cfm_dev.h", "cfm.hip", "gcd.hip"))
    assert "constexpr int kGroups = kBlock / kG;" in dev
    assert "for (int64_t t = threadIdx.x; t < np; t += kNarrowBlock) a += part[t];" in dev  # fin_sum
    assert "for (int64_t c = q0; c < q1; c += kG)" in dev and "if (c + u < q1) acc += tu;" in dev  # ordered_acc
    assert "inline size_t pad32(size_t v)" in dev and "pad32(S->d + 1)" in dev
    assert 'getenv("NFM_HAZAN_GRAPH")' in cfm and cfm.count("for (int c = 0; c < kHazanChunk; ++c) issue();") == 2
    assert "done < max_iter_power + kHazanChunk" in cfm and "done < kCgMaxIter + kHazanChunk" in cfm
    assert "it >= (double)kCgMaxIter" in cfm
    assert hr.CG_MAX_ITER == kCgMaxIter
    # the callers of fin_sum and the counts they pass: the table below restates exactly these
    for text, kernel, count in ((cfm, "k_power_fin, 1, kNarrowBlock, Pt.p0, Pt.p1, gd", 1), (cfm, "k_step, 1, kNarrowBlock, Pt.p0, Pt.p1, gn", 1),
                                (cfm, "k_cg_bfin, 1, kNarrowBlock, Pt.p0, gd, Pt.p3, en", 1), (cfm, "k_cg_apd, 1, kNarrowBlock, Pt.p2, gn", 1),
                                (cfm, "k_cg_curv, 1, kNarrowBlock, Pt.p2, gn, Pt.p0, gd", 1), (cfm, "k_cg_init3, 1, kNarrowBlock, Pt.p0, gz", 1),
                                (cfm, "k_cg_beta, 1, kNarrowBlock, Pt.p0, Pt.p1, gz", 1), (cfm, "k_icpt, 1, kNarrowBlock, Pt.p3, en", 1),
                                (cfm, "k_loss, 1, kNarrowBlock, Pt.p0, en", 2), (gcd, "k_gcd_fitlams, 1, kNarrowBlock, Pt.p0, Pt.p1, gn", 1),
                                (gcd, "k_gcd_fitlams, 1, kNarrowBlock, Pt.p0, Pt.p1, en", 1),
                                (gcd, "k_gcd_obj, 1, kNarrowBlock, Pt.p0, en, Pt.p1, outer ? ed : (int64_t)-1", 1)):
        assert text.count(kernel) == count, kernel
    assert "gn = blocks_for(n, kGroups), gd = blocks_for(d, kGroups), en = blocks_for(n, kBlock), ed = blocks_for(d, kBlock)" in cfm
    assert "gz = blocks_for(dz, kBlock)" in cfm


def partials(name, fitIntercept=True):
    """the workgroup counts of the passes over one input: what each caller of fin_sum gets as its number of partials"""
    n, d = G.SHAPES[name][:2]
    dz = d + (1 if fitIntercept else 0)
    c = dict(n=n, d=d, dz=dz, gn=ceil_div(n, kGroups), gd=ceil_div(d, kGroups), en=ceil_div(n, kBlock), ed=ceil_div(d, kBlock),
             gz=ceil_div(dz, kBlock))
    # caller -> the counts of the sums it finishes
    c["callers"] = {"k_power_fin": (c["gd"],), "k_step": (c["gn"],), "k_cg_bfin": (c["gd"], c["en"]), "k_cg_apd": (c["gn"],),
                    "k_cg_curv": (c["gn"], c["gd"]), "k_cg_init3": (c["gz"],), "k_cg_beta": (c["gz"],), "k_icpt": (c["en"],),
                    "k_loss": (c["en"],), "k_gcd_fitlams new base": (c["gn"],), "k_gcd_fitlams refit": (c["en"],),
                    "k_gcd_obj": (c["en"], c["ed"])}
    c["trips"] = {k: tuple(ceil_div(v, kNarrowBlock) for v in vs) for k, vs in c["callers"].items()}
    return c


def test_tall_reaches_the_second_trip_over_the_row_partials():
    c = partials("tall")
    assert c["gn"] == kNarrowBlock + 2 and c["n"] - (c["gn"] - 1) * kGroups == 1  # the last workgroup holds one row
    for caller in ("k_step", "k_cg_apd", "k_gcd_fitlams new base"):
        assert c["trips"][caller] == (2,), caller
    assert c["trips"]["k_cg_curv"] == (2, 1)  # sum of Xp over the rows; p . Ap over 2 workgroups of columns
    assert c["en"] < kNarrowBlock and c["gd"] == 2  # nothing else takes a second trip here: `long` and `broad` do
    assert c["n"] % kBlock not in (0, kBlock - 1)


def test_long_reaches_the_second_trip_over_the_element_wise_partials():
    c = partials("long")
    assert c["en"] == kNarrowBlock + 2 and c["n"] - (c["en"] - 1) * kBlock == 1
    for caller in ("k_loss", "k_icpt", "k_gcd_fitlams refit"):
        assert c["trips"][caller] == (2,), caller
    assert c["trips"]["k_cg_bfin"] == (1, 2) and c["trips"]["k_gcd_obj"] == (2, 1)
    assert c["trips"]["k_step"] == (ceil_div(c["gn"], kNarrowBlock),) and c["trips"]["k_step"][0] >= 9  # and many over the rows
    X, _ = G.data("long")
    assert 390000 < len(X.rval) < 410000
    assert G.GCD["nRefitting"] <= G.GCD["maxIterInner"] and "long:11" in G.GCD_CASES  # refitDiag runs on `long`
    a, _ = gcd_fits("long:11")
    assert any(r["refit"] and r["nComponents"] > 0 for o in a.history for r in o["inner"])
    kw = G.hazan_kw("long", (True, True, True, True))
    assert kw["maxIter"] <= 2 and kw["maxIterPower"] <= 8
    assert ("long", (True, True, False, True)) in G.HAZAN_RUNS  # k_icpt


def test_broad_puts_mass_behind_partial_1024_of_the_passes_over_d():
    c = partials("broad")
    assert c["dz"] == c["d"] + 1 == 262402
    assert c["trips"]["k_power_fin"] == (9,) and c["trips"]["k_cg_curv"] == (1, 9) and c["trips"]["k_cg_bfin"] == (9, 1)
    assert c["ed"] == c["gz"] == kNarrowBlock + 2  # d = 256 * 1025 + 1: column d - 1 and the dummy column share the last workgroup
    assert c["trips"]["k_cg_init3"] == c["trips"]["k_cg_beta"] == (2,) and c["trips"]["k_gcd_obj"] == (1, 2)
    used = G.SHAPES["broad"][2]
    assert len(used) == 104 and sorted(set(used // kGroups)) == [0, 1, kNarrowBlock, 8 * kNarrowBlock]  # the column pass's partials
    assert sorted(set(used // kBlock)) == [0, 128, kNarrowBlock]  # the element-wise passes': only the far band is past 1024
    X, _ = G.data("broad")
    assert set(np.unique(X.ridx)) == set(used)
    far = slice(G.BROAD_BANDS[2][0], G.BROAD_BANDS[2][1])
    for name, flags in G.HAZAN_RUNS:
        if name != "broad":
            continue
        run = G.hazan_plain(name, flags)
        shareP = np.abs(run.P[:, far]).max() / np.abs(run.P).max()
        shareW = np.abs(run.w[far]).max() / np.abs(run.w).max() if flags[2] else 1.0
        print("broad %s: the far band holds %.3f of max |P| and %.3f of max |w|; CG %s" % (flags, shareP, shareW,
                                                                                           [r["cgIters"] for r in run.history]))
        assert shareP >= 0.01 and shareW >= 0.01  # a dropped trip cannot hide inside the tolerance
    a, _ = gcd_fits("broad:11")
    assert np.abs(a.P[:, far]).max() / np.abs(a.P).max() >= 0.01 and np.abs(a.w[far]).max() / np.abs(a.w).max() >= 0.01


def test_edge_shapes_sit_on_the_workgroup_edges():
    assert sorted(G.SHAPES["edges_n%d" % n][0] % kGroups for n in G.EDGES_N) == [0, 0, 1, 1, kGroups - 1, kGroups - 1]
    assert [n - kGroups for n in G.EDGES_N[:3]] == [-1, 0, 1] and [n - kBlock for n in G.EDGES_N[3:]] == [-1, 0, 1]
    for n in G.EDGES_N:
        c = partials("edges_n%d" % n)
        assert (c["gn"], c["en"]) == (ceil_div(n, kGroups), ceil_div(n, kBlock)) and c["d"] == 33
    assert [partials("edges_n%d" % n)["en"] for n in G.EDGES_N] == [1, 1, 1, 1, 1, 2]
    assert [partials("edges_n%d" % n)["gn"] for n in G.EDGES_N] == [1, 1, 2, 8, 8, 9]
    # the CG's sums over the rows run on the three larger ones, which leave the same remainders of a workgroup's rows
    for n in G.EDGES_N:
        flags = dict(G.HAZAN_RUNS)["edges_n%d" % n]
        assert flags[3] and flags[2] == (n > 33)
    assert [d + 1 - kGroups for d in G.EDGES_D[:2]] == [0, 1] and [d + 1 - kBlock for d in G.EDGES_D[2:]] == [0, 1]
    for d in G.EDGES_D:
        c = partials("edges_d%d" % d)
        assert dict(G.HAZAN_RUNS)["edges_d%d" % d][2:] == (True, True)  # the linear part with the intercept: dz = d + 1
        assert c["gz"] - c["ed"] == (1 if d % kBlock == 0 else 0)  # the dummy column alone in a workgroup of its own
    assert partials("edges_d255")["dz"] == kBlock and partials("edges_d256")["gz"] == 2
    pad32 = lambda v: (v + 31) // 32 * 32
    assert [pad32(d + 1) - d for d in G.EDGES_D] == [1, 32, 1, 32]  # the dummy slot: the last of its line / the first of a new one


def test_row_lengths():
    """every row length of the cycle is there, in particular every remainder of kG that ordered_acc's last round can meet"""
    want = {name: set(G.CYCLE) | {min(200, len(G.SHAPES[name][2]))} for name in G.SHAPES if G.SHAPES[name][3] == G.CYCLE}
    want["long"] = set(G.LONG_CYCLE) | {39}
    want["cg_long"] = want["cg_cap"] = {8}
    assert set(want) == set(G.SHAPES)
    last = {"tall": 9, "long": 1, "broad": 16}  # the last row, the only one of the last workgroup on tall and long
    for name, lens_want in want.items():
        X, _ = G.data(name)
        lens = np.diff(X.rptr)
        assert set(lens.tolist()) == lens_want, name
        if name in last:
            assert lens[-1] == last[name] == G.SHAPES[name][3][(X.n - 1) % len(G.SHAPES[name][3])], name
        if G.SHAPES[name][4] is not None:
            assert lens[G.LONG_ROW] == max(lens_want) and np.abs(X.rval[X.rptr[G.LONG_ROW]:X.rptr[G.LONG_ROW + 1]]).max() <= 0.15
        nz = lens > 0
        assert (X.ridx[X.rptr[:-1][nz]] == 0).all()  # column 0 holds every non-empty row
        col0 = np.abs(X.rval[X.rptr[:-1][nz]])
        assert ((col0 >= 0.2) & (col0 <= 1.0) | (np.arange(X.n)[nz] == G.LONG_ROW)).all()
        for i in range(min(X.n, 64)):  # ascending, distinct column ids
            assert (np.diff(X.ridx[X.rptr[i]:X.rptr[i + 1]]) > 0).all()
    assert {l % kG for l in G.CYCLE} == {0, 1, 3, 7} and {l // kG for l in G.CYCLE} == {0, 1, 2}
    assert set(G.CYCLE) >= {0, 1, kG - 1, kG, kG + 1, 2 * kG - 1, 2 * kG, 2 * kG + 1}
    X, _ = G.data("tall")
    assert X.n == kGroups * (kNarrowBlock + 1) + 1 and not (X.ridx == X.d - 1).any()  # the last column is empty
    X, _ = G.data("long")
    assert X.n == kBlock * (kNarrowBlock + 1) + 1


def test_the_predict_cases():
    X, _ = G.data("predict33")
    assert (X.n, X.d) == (33, G.SHAPES["tall"][1]) and set(np.diff(X.rptr).tolist()) == set(G.CYCLE) | {39}
    models = G.predict_models(X.d, G.SHAPES["tall"][2])
    assert [len(m[1]) for m in models] == [0, 1, 3]


# ---- the conditioning guards, with the rules of tests/test_hazan_restatement.py and tests/test_gcd_restatement.py ----
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300)) if a.size else 0.0


def _guard(X, y, starts, kw, run):
    """tests/test_hazan_restatement.py's _guard"""
    forced = [(r["powerIters"], r["cgIters"]) for r in run.history]
    tree = hr.hazan_fit(X, y, starts, summation="tree", forced=forced, **kw)
    worst = max(_rel(tree.P, run.P), _rel(tree.lams, run.lams), _rel(tree.w, run.w),
                max(abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(tree.history, run.history)))
    assert [a["slot"] for a in tree.history] == [b["slot"] for b in run.history]
    print("tree against in-order sums: %.2e" % worst)
    assert worst < 1e-8, worst


@pytest.mark.parametrize("name,flags", G.HAZAN_RUNS, ids=["%s-%s" % (n, "".join("FT"[f] for f in fl)) for n, fl in G.HAZAN_RUNS])
def test_hazan_conditioning_guard(name, flags):
    X, y, kw, starts = G.hazan_case(name, flags)
    assert kw["maxIter"] <= 4 and kw["maxIterPower"] <= 40
    _guard(X, y, starts, kw, G.hazan_plain(name, flags))


@pytest.mark.parametrize("maxIterPower", G.POWER_EDGES)
def test_hazan_conditioning_guard_power_edges(maxIterPower):
    X, y, kw, starts = G.hazan_case("grid", G.POWER_EDGE_FLAGS, maxIterPower=maxIterPower)
    run = G.hazan_plain("grid", G.POWER_EDGE_FLAGS, maxIterPower)
    assert kw["tolPower"] == 0.0 and kw["maxIter"] == 2 and [r["powerIters"] for r in run.history] == [maxIterPower] * 2
    _guard(X, y, starts, kw, run)
    assert {m % kHazanChunk for m in G.POWER_EDGES} == {1, kHazanChunk - 1, 0} and max(G.POWER_EDGES) == 2 * kHazanChunk + 1
    assert G.GCD_POWER_EDGE == kHazanChunk + 1


def test_cg_long_runs_past_one_chunk():
    name, flags = G.CG_LONG_RUN
    X, y, kw, starts = G.hazan_case(name, flags)
    assert kw["maxIter"] == 1
    run = G.hazan_plain(name, flags)
    tree = hr.hazan_fit(X, y, starts, summation="tree", **kw)
    for r in (run.history[0], tree.history[0]):
        print("cg_long: %d CG iterations, ||r||_1 / tol at the stop %.3g, one earlier %.3g" % (r["cgIters"], r["cgNorm"] / r["cgTol"],
                                                                                            r["cgNormPrev"] / r["cgTol"]))
        assert kHazanChunk + 1 <= r["cgIters"] <= 60 and 33 <= r["cgIters"]
    assert run.history[0]["cgIters"] - 1 > kHazanChunk  # the device may stop one earlier and still be in the second chunk
    _guard(X, y, starts, kw, run)


def test_cg_cap_ends_on_the_cap_with_a_margin():
    """no parity on this input, only the robust facts: under both summations the CG is still at least 10x above its
    tolerance after kCgMaxIter iterations, and everything is finite; measured here 39x (in order) and 35x (trees), with the
    two results 6.3e-5 apart on w -- a CG that long is chaotic under rounding, which is why nothing else is compared"""
    name, flags = G.CG_CAP_RUN
    X, y, kw, starts = G.hazan_case(name, flags)
    assert kw["maxIter"] == 1 and X.d > 2 * X.n
    runs = [G.hazan_plain(name, flags), hr.hazan_fit(X, y, starts, summation="tree", **kw)]
    for run in runs:
        r = run.history[0]
        print("cg_cap: %d CG iterations, ||r||_1 / tol %.3g" % (r["cgIters"], r["cgNorm"] / r["cgTol"]))
        assert r["cgIters"] == kCgMaxIter and r["cgNorm"] >= 10.0 * r["cgTol"]
        assert np.isfinite(run.w).all() and np.isfinite(run.P).all() and np.isfinite(r["loss"]) and np.isfinite(run.intercept)
    print("cg_cap: tree against in-order sums on w: %.2e" % _rel(runs[1].w, runs[0].w))
    assert kCgMaxIter % kHazanChunk != 0  # the cap falls inside a chunk: the launches after it must do nothing


@functools.lru_cache(maxsize=None)
def gcd_fits(name):
    """(in-order sums, the device's trees forced to the same discrete decisions) of one case, computed once"""
    X, y, kw = G.gcd_case(name)
    st = G.hc.numpy_starts(G.START_SEED)
    a = gr.gcd_fit(X, y, st, summation="order", **kw)
    b = gr.gcd_fit(X, y, st, summation="tree", forced=gr.counts_of(a.history), **kw)
    return a, b


def _inner(res):
    return [r for o in res.history for r in o["inner"]]


@pytest.mark.parametrize("name", G.GCD_CASES + [G.GCD_GRID_CASE])
def test_gcd_conditioning_guard(name):
    """tests/test_gcd_restatement.py's test_conditioning_guard"""
    a, b = gcd_fits(name)
    T = gc.TOL
    assert a.P.shape == b.P.shape and [(r["slot"], r["added"]) for r in _inner(a)] == [(r["slot"], r["added"]) for r in _inner(b)]
    rP = (np.abs(a.P - b.P) / (T["P_atol"] + T["P_rtol"] * np.abs(a.P))).max()
    rw = (np.abs(a.w - b.w) / (T["w_atol"] + T["w_rtol"] * np.abs(a.w))).max()
    rl = np.abs(a.lams - b.lams).max() / T["lams_atol"]
    rb = abs(a.intercept - b.intercept) / T["intercept_atol"]
    oa = np.array([r["objective"] for r in _inner(a)] + [o["loss"] + o["reg"] for o in a.history])
    ob = np.array([r["objective"] for r in _inner(b)] + [o["loss"] + o["reg"] for o in b.history])
    ro = (np.abs(oa - ob) / np.abs(oa)).max() / T["obj_rtol"]
    print("%s: fraction of the tolerance  P %.2e  w %.2e  lams %.2e  intercept %.2e  objectives %.2e" % (name, rP, rw, rl, rb, ro))
    assert max(rP, rw, rl, rb, ro) <= 1e-2
    _, _, kw = G.gcd_case(name)
    assert kw["maxIterPower"] <= 40 and any(r["refit"] for r in _inner(a))
    powers = [r["powerIters"] for r in _inner(a) if r["slot"] >= 0]
    assert powers and all(p == kw["maxIterPower"] for p in powers)  # tolPower = 0: the cap ends every power method
    if not name.startswith("grid"):
        assert np.count_nonzero(a.lams) == kw["maxComponents"]


def test_the_empty_column_shortcut_of_the_gcd_restatement_changes_nothing():
    """gcd_restatement skips an empty column whose w is zero (its update is an * 0 / inv): with the shortcut disabled by a
    stored explicit zero in every empty column the fit is the same to the bit"""
    X, y = G.hc.grid_data(True, True)
    d2 = X.d + 3
    wide = hr.Data(X.rptr, X.ridx, X.rval, X.n, d2)  # three empty columns
    kw = dict(gc.GRID, maxIter=2, maxIterInner=3, nRefitting=2, ignoreDiag=True, fitLinear=True, fitIntercept=True)
    st = lambda k, d: G.hc.numpy_starts(G.START_SEED)(k, d2)
    a = gr.gcd_fit(wide, y, st, **kw)
    lens = np.diff(X.rptr)
    idx, val, ptr = [], [], [0]
    for i in range(X.n):  # the same matrix with explicit zeros in column d (so that column is not empty)
        idx += list(X.ridx[X.rptr[i]:X.rptr[i + 1]]) + [X.d]
        val += list(X.rval[X.rptr[i]:X.rptr[i + 1]]) + [0.0]
        ptr.append(ptr[-1] + int(lens[i]) + 1)
    b = gr.gcd_fit(hr.Data(ptr, idx, val, X.n, d2), y, st, **kw)
    assert a.w.tobytes() == b.w.tobytes() and a.lams.tobytes() == b.lams.tobytes() and not a.w[X.d:].any()
