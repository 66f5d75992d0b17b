"""CPU: the conditions the large-grid inputs of tests/dense_grid_cases.py must meet so that the GPU tests built on them
(test_large_grids in tests/test_gpu_pgd.py, the GRID_CASES of tests/katyusha_cases.py, the grid cases of tests/test_gpu_psgd.py)
reach the code they are there for and may keep the tolerances of their files.  No GPU: the restatements and the oracle only.

Coverage is asserted, not claimed: the caps of the grid-stride loops are read out of the sources, and every trip count and
workgroup count the GPU tests rely on is recomputed from them, so a later retune of a cap fails here instead of silently
ending the coverage.

Spread of the restatements between sequential and pairwise sums (and, for Katyusha, the pivoting and the sort-based prox),
measured here: PGD family 0 (tall_pgd_l1, tall_fista_sql21, deep_pgd_sql12_row, deep_fista_sql12_col), 6.3e-14
(tall_nmapgd_sql12_col), 2.2e-13 (deep_nmapgd_l21); Katyusha at most 6.3e-16 on the parameters and 2.8e-14 on viol and
lossVal.  All are below 1e-11, a tenth of the tightest device tolerance, so no tolerance is widened."""
import math
import os
import re

import numpy as np
import pytest

import dense_grid_cases as G
import katyusha_cases as Kc
import pgd_restatement as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")


def _const(name, file):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, file)).read())
    assert m, (name, file)
    return int(m.group(1))


kWave, kBlock = _const("kWave", "common.h"), _const("kBlock", "common.h")
kPgdMaxBlocks = _const("kPgdMaxBlocks", "pgd.h")
kPassBlocks, kProxBlock, kPasses = _const("kPassBlocks", "psgd.hip"), _const("kProxBlock", "psgd.hip"), _const("kPasses", "psgd.hip")
N_CU = 256  # k_pgd_mix's cap is 16 workgroups per compute unit: asserted for the 256 CUs of an MI355X, other parts differ


def ceil_div(a, b):
    return -(-a // b)


def geometry(shape):
    k, d, n, m = G.SHAPES[shape]
    L = G.lanes_for_k(k)
    return dict(k=k, d=d, da=d, L=L, Kp=2 * L, R=kWave // L, rows_per_wg=(kBlock // kWave) * (kWave // L))


def row_trips(da, rows_per_wg, cap, d=0):
    """(workgroups, trips, rows of the last trip) of a row loop  j0 += gridDim.x * kWavesPerBlock * R  under a cap"""
    g = min(cap, max(ceil_div(max(da, d), rows_per_wg), 1))
    per_trip = g * rows_per_wg
    trips = ceil_div(da, per_trip)
    return g, trips, da - (trips - 1) * per_trip


def test_the_source_still_has_the_loops_these_numbers_describe():
    pgd, kat, psgd = (open(os.path.join(CSRC, f)).read() for f in ("pgd.hip", "katyusha.hip", "psgd.hip"))
    for text in (pgd, kat):
        assert "j0 < M.da; j0 += stride" in text and "gridDim.x * kWavesPerBlock * R" in text
        assert "j < M.d; j += (int64_t)gridDim.x * kBlock" in text
    assert "std::min<int64_t>(kPgdMaxBlocks, need)" in pgd and "(int64_t)ctx->n_cu * 16" in pgd
    assert "for (int g = lane; g < f.G; g += kWave)" in pgd
    assert "M.da <= 16 * kProxBlock" in psgd and "std::min<int64_t>(kPassBlocks," in psgd and "r < M.da; r += stride" in psgd
    assert G.lanes_for_k(2) == 1 and G.lanes_for_k(3) == 2 and G.lanes_for_k(33) == 32 and G.lanes_for_k(127) == 64 and G.lanes_for_k(128) == 64


def test_tall_and_deep_reach_the_second_trips():
    t, dp = geometry("tall"), geometry("deep")
    assert (t["L"], t["Kp"]) == (1, 2) and (dp["L"], dp["Kp"]) == (64, 128) and dp["k"] == dp["Kp"] - 1  # one padding column
    # k_pgd_trial<L> / k_kat_dense<L> rows: the capped grid, a second (third) trip, a partial last wavefront (workgroup)
    g, trips, last = row_trips(t["da"], t["rows_per_wg"], kPgdMaxBlocks, t["d"])
    assert g == kPgdMaxBlocks > kWave and trips == 2 and last == 156
    assert last // t["R"] == 2 and 0 < last % t["R"] < t["R"]  # two full wavefronts and a partial one
    g, trips, last = row_trips(dp["da"], dp["rows_per_wg"], kPgdMaxBlocks, dp["d"])
    assert g == kPgdMaxBlocks > kWave and trips == 3 and last == 9 and last % dp["rows_per_wg"] != 0
    # the linear part of the same kernels: j += gridDim.x * kBlock
    assert t["d"] > kPgdMaxBlocks * kBlock
    for s in (t, dp):
        nP = s["da"] * s["Kp"]
        # k_pgd_bb, k_kat_end: the flat loops under the same cap
        flat_g = min(kPgdMaxBlocks, ceil_div(max(nP, s["d"]), kBlock))
        assert flat_g == kPgdMaxBlocks > kWave and ceil_div(nP, flat_g * kBlock) >= 2
    assert t["da"] * t["Kp"] == 524600 and dp["da"] * dp["Kp"] == 1049728
    assert ceil_div(t["da"] * t["Kp"], kPgdMaxBlocks * kBlock) == 3  # the Barzilai-Borwein sums over 3 trips
    # k_pgd_mix: 16 workgroups per CU, at 256 CUs
    assert dp["da"] * dp["Kp"] > kBlock * 16 * N_CU
    # launch_prox_coupled's row-parallel path from PGD (tall), and k_psgd_prox_norms / the rescale over many rows
    assert t["da"] > 16 * kProxBlock >= dp["da"]
    g, trips, last = row_trips(t["da"], t["rows_per_wg"], kPassBlocks)
    assert g == kPassBlocks and trips == 2
    assert Kc.GRID_CASES["wide_l1_k130"]["data"]()[2].shape[1] == 130 > 128  # kc = 2 device blocks


def test_passes_and_vpt_land_where_they_should():
    p = geometry("passes")
    assert (p["L"], p["Kp"]) == (32, 64) and p["da"] > 16 * kProxBlock
    g, trips, last = row_trips(p["da"], p["rows_per_wg"], kPassBlocks)
    assert g == kPassBlocks and trips >= 2
    instance = lambda vpt: next(v for v in (1, 2, 4, 8, 16) if vpt <= v)  # launch_psgd_step_t's ladder
    want = {1500: 2, 6000: 8, 12000: 16, 16384: 16}
    for d in G.VPT_D:
        s = geometry("vpt%d" % d)
        assert s["L"] == 2
        if d in want:
            assert d <= 16 * kProxBlock and instance(ceil_div(d, kProxBlock)) == want[d]
        else:
            assert d == 16 * kProxBlock + 1  # the first size on the row-parallel path
    assert 16384 == 16 * kProxBlock


def rel_margin(a, b):
    m = max(abs(a), abs(b))
    return 1.0 if not (math.isfinite(a) and math.isfinite(b)) or m == 0.0 else abs(a - b) / m


@pytest.mark.parametrize("name", list(G.PGD_CASES))
def test_pgd_case_conditions(name):
    shape, algo, skw, iters, scale = G.PGD_CASES[name]
    assert iters in (2, 3)
    s, r = G.pgd_restate(name)
    assert r.margins and min(rel_margin(a, b) for a, b in r.margins) >= 1e-6
    share = float((r.P == 0.0).mean())
    print("%s zeros %.3f" % (name, share))
    assert 0.05 < share < 0.95, (name, share)
    s2, r2 = G.pgd_restate(name, "pair")
    assert [(i["trials"], i["branch"]) for i in r.iters] == [(i["trials"], i["branch"]) for i in r2.iters], name
    spread = max(np.abs(r.P - r2.P).max() / np.abs(r.P).max(), np.abs(r.w - r2.w).max(), abs(r.b - r2.b))
    print("spread %-24s %.3e" % (name, spread))
    assert spread <= 1e-11, (name, spread)  # a tenth of 1e-10, the tighter of the two tolerances of tests/test_gpu_pgd.py
    assert np.array_equal(r.P == 0.0, r2.P == 0.0)
    for a, b in zip(r.iters, r2.iters):
        for key in ("lossVal", "regVal", "viol", "c"):
            assert abs(a[key] - b[key]) <= 1e-11 * abs(a[key]), (name, key)
    assert set(G.PGD_BITWISE) <= set(G.PGD_CASES) and {G.PGD_CASES[n][0] for n in G.PGD_BITWISE} == {"tall", "deep"}


@pytest.mark.parametrize("name", list(Kc.GRID_CASES))
def test_katyusha_case_conditions(name):
    c = Kc.GRID_CASES[name]
    s, r = Kc.restate(name)
    assert r.inner == (5 if name == "wide_l1_k130" else r.inner) and (name == "wide_l1_k130" or r.inner in (2, 3))
    assert len(r.iters) == c["max_iter"] in (1, 2)
    for kw in (dict(sums="pair"), dict(sums="pair", prox="slow")):  # both switches; the bound of tests/test_katyusha_restatement.py
        q = Kc.restate(name, **kw)[1]
        spread = max(np.abs(r.P - q.P).max() / np.abs(r.P).max(), np.abs(r.w - q.w).max(), abs(r.b - q.b))
        print("spread %-20s %-32s %.3e" % (name, kw, spread))
        assert spread <= 1e-11, (name, kw, spread)
        assert np.array_equal(r.P == 0.0, q.P == 0.0), (name, kw)
        for a, b in zip(r.iters, q.iters):
            assert abs(a["viol"] - b["viol"]) <= 1e-11 * abs(a["viol"]) and abs(a["lossVal"] - b["lossVal"]) <= 1e-11 * abs(a["lossVal"])
    # delta is not small: a gradient taken at one parameter set only, or at unstamped rows only, cannot pass
    assert r.iters[-1]["delta_ratio"] >= 1e-3
    Xo, y, P0 = Kc.inputs(name)[:3]
    zP = r.z.P.transpose(0, 2, 1)
    share = float((zP[P0 != 0.0] == 0.0).mean())  # what the prox zeroed of z where the start was not zero
    print("%s z zeros %.3f P zeros %.3f" % (name, share, (r.P == 0.0).mean()))
    assert 0.05 < share < 0.95, (name, share)
    if name == "wide_l1_k130":
        return
    assert 0.05 < float((r.P == 0.0).mean()) < 0.95
    touched = np.zeros(P0.shape[2], dtype=bool)
    touched[np.unique(Xo.indices)] = True
    assert touched.mean() < 0.2  # most features are never stamped
    tz = touched & (P0[0, 0] == 0.0)
    left = float((r.P[:, :, tz] != 0.0).mean())  # touched rows that start at zero: the final zero pattern is the prox's decision
    print("%s touched rows starting at zero: %d, entries that left zero %.3f" % (name, tz.sum(), left))
    if name != "tall_sql21":  # its threshold outweighs every gradient step (katyusha_cases.py): the pattern there is the start's
        assert 0.0 < left < 1.0


@pytest.mark.parametrize("name", list(G.PSGD_CASES))
def test_psgd_case_conditions(name):
    shape, gamma, B, outer = G.PSGD_CASES[name]
    P, w, b = G.psgd_oracle(name)
    share = float((P == 0.0).mean())
    print("%s zeros %.4f" % (name, share))
    assert (P != 0.0).any()
    P0 = G.data(shape, G.PSGD_SCALE)[2]
    lam = gamma * 0.2 / (1.0 + 0.2 * 1e-2)  # the largest lam of check()'s schedule (eta0 = 0.2, beta = 1e-2)
    passes = [G.threshold_passes(P0[0, s], lam) for s in range(P0.shape[1])]  # on the start's columns: the first mini-batch's, nearly
    if name == "passes_finish":  # exempt from the share rule by what it is for (dense_grid_cases.py)
        assert min(passes) > kPasses
    else:
        assert 0.05 < share < 0.95, (name, share)
        assert max(passes) <= kPasses


def test_vectorised_sequential_sum_is_the_loop():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(10 ** 6) * np.exp(rng.uniform(-20, 20, 10 ** 6))
    b = rng.standard_normal(10 ** 6)
    c = np.concatenate([b, -b])[rng.permutation(2 * 10 ** 6)][:10 ** 6] * 1e8  # cancelling: the total is far below the terms
    c[::1000] += 1e-8
    for v in (a, b, c, np.zeros(0), np.array([-0.0]), np.array([1e300, 1.0, -1e300])):
        want, got = R.seq_sum_loop(v), R.seq_sum(v)
        assert np.float64(want).tobytes() == np.float64(got).tobytes()
    assert R.seq_sum(c) != R.pair_sum(c)  # the order matters on this input, and the sequential one is kept
