"""The route of a field-aware mini-batch (nimfm_amd/csrc/mb_ffm_route.h: which row kernel with how much LDS, whether k_ffm_refresh
runs, every grid size, where each kernel's partials sit, the work buffers' bounds, the LDS layout of k_ffm_row_phase_lds) is plain
C++: tests/cpp/mb_ffm_route_test.cpp builds with g++ alone -- no HIP, no library -- reads cases on stdin and prints the header's
answers.  They are held against the restatement of tests/ffm_kernel_cases.py (row kernel, refresh), against the grids restated
below, and the bounds against the routes they must hold and against the formulas mb_ffm_epoch had of its own.  Built the way
tests/test_cpp_mb_route.py builds its program; a second build with -fsanitize=address,undefined runs the same input stand-alone."""
import collections
import functools
import os
import subprocess

import numpy as np

import ffm_kernel_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mb_ffm_route_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_mb_ffm_route_test")
UNSET = -2147483648
SGD, ADAGRAD = 0, 1  # mb_route.h: MB_SGD, MB_ADAGRAD
LS = (1, 2, 4, 8, 16, 32, 64)
KERNELS = ("generic", "lds", "coop")  # mb_ffm_route.h: FFM_ROW_GENERIC, FFM_ROW_LDS, FFM_ROW_COOP

Shape = collections.namedtuple("Shape", "L opt nb Kp max_row first_singleton")
Knobs = collections.namedtuple("Knobs", "lds refresh", defaults=(None, None))
Batch = collections.namedtuple("Batch", "b len uniq touches heavy segs")
Maxima = collections.namedtuple("Maxima", "batch unique touch heavy segs")


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def line(S, Kn, B, M=None):
    M = Maxima(B.len, B.uniq, B.touches, B.heavy, B.segs) if M is None else M
    return " ".join(str(int(UNSET if v is None else v)) for v in tuple(S) + tuple(Kn) + tuple(B) + tuple(M))


def run(lines, sanitize=False):
    out = subprocess.run([exe(sanitize)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) and "%d cases" % len(lines) in out.stderr
    return [parse(ln) for ln in got]


def parse(ln):
    row, lds, route, bounds, consts = (part.split() for part in ln.split("|"))
    g = {"kernel": KERNELS[int(row[0])], "lds_bytes": int(row[1]), "wpb": int(row[2]), "big": int(row[3]), "m_cap": int(row[4]), "counter": row[5]}
    g["layout"] = dict(zip(("rows", "fmask", "xs", "js", "fs", "per_wave"), map(int, lds)))
    g.update(zip(("refresh", "use_stored", "nA", "nR", "nB", "nsb", "nH", "off_refresh", "off_col", "off_heavy", "n_parts"), map(int, route)))
    g["bounds"] = dict(zip(("contrib", "rec", "partsA", "partsB", "hpart"), map(int, bounds)))
    g["consts"] = (int(consts[0]), int(consts[1]), consts[2])
    return g


ONE = Batch(1, 1, 1, 1, 0, 0)  # where only the epoch call's shape is asked about


# ---------------------------------------------------------------- the row kernel, the LDS layout, the two constants
def check_row(g, k, F, max_row, what):
    kernel, lds_bytes = K.row_kernel(k, F, max_row)
    assert (g["kernel"], g["lds_bytes"]) == (kernel, lds_bytes), what
    assert g["counter"] == K.FAMILY[kernel] and g["big"] == int(lds_bytes > K.LDS_DEFAULT) and g["m_cap"] == max(max_row, 1), what
    assert g["wpb"] == (1 if kernel == "coop" else 4), what


def test_the_row_kernel_of_every_case_is_the_restatements():
    shapes = [Shape(K.lanes_for_k(c.k), opt, c.F, 2 * K.lanes_for_k(c.k), max(c.lengths), 0) for c in K.ROW_CASES for opt in (SGD, ADAGRAD)]
    got = run([line(S, Knobs(), ONE) for S in shapes])
    for i, g in enumerate(got):
        c = K.ROW_CASES[i // 2]
        check_row(g, c.k, c.F, max(c.lengths), c.name)
        assert (g["kernel"], g["lds_bytes"]) == (c.kernel, c.lds_bytes), c.name
    assert {g["consts"] for g in got} == {(K.LDS_SHARE, K.LDS_DEFAULT, K.BIG)}


@functools.lru_cache(maxsize=None)
def grid():
    """Kp x F x max_row; a model of k = Kp components has Kp / 2 lanes per row and no padding"""
    cs = [(Kp, F, m) for Kp in (2, 4, 8, 16, 32, 64, 128) for F in range(1, 66) for m in range(0, 66)]
    assert all(2 * K.lanes_for_k(Kp) == Kp for Kp, _, _ in cs)
    return cs, run([line(Shape(Kp // 2, SGD, F, Kp, m, 0), Knobs(), ONE) for Kp, F, m in cs])


def test_the_row_kernel_over_the_whole_grid():
    cs, got = grid()
    seen = set()
    for (Kp, F, m), g in zip(cs, got):
        check_row(g, Kp, F, m, (Kp, F, m))
        seen.add((g["kernel"], g["big"], Kp))
    assert seen >= {(kn, big, Kp) for kn in ("lds", "coop") for big in (0, 1) for Kp in (8, 16, 32, 64, 128)} | {("generic", 0, Kp) for Kp in (2, 128)}
    off = run([line(Shape(Kp // 2, SGD, F, Kp, m, 0), Knobs(lds=0), ONE) for Kp, F, m in cs])
    assert {(g["kernel"], g["lds_bytes"], g["wpb"], g["big"], g["counter"]) for g in off} == {("generic", 0, 4, 0, "ffm_row_generic")}
    assert [g["m_cap"] for g in off] == [max(m, 1) for _, _, m in cs]
    on = run([line(Shape(Kp // 2, SGD, F, Kp, m, 0), Knobs(lds=1), ONE) for Kp, F, m in cs[::7]])  # any other value: as unset
    assert [(g["kernel"], g["lds_bytes"]) for g in on] == [(g["kernel"], g["lds_bytes"]) for g in got[::7]]


def test_the_lds_layout_holds_its_five_arrays():
    cs, got = grid()
    for (Kp, F, m), g in zip(cs, got):
        lo, m_cap = g["layout"], max(m, 1)
        ends = [("rows", m_cap * F * Kp * 8, 16), ("fmask", F * 8, 8), ("xs", m_cap * 8, 8), ("js", m_cap * 4, 4), ("fs", m_cap * 4, 4)]
        at = 0
        for name, size, align in ends:  # in this order, none over the one before, each aligned
            assert lo[name] >= at and lo[name] % align == 0, (Kp, F, m, name, lo)
            at = lo[name] + size
        assert at <= lo["per_wave"] and lo["per_wave"] % 16 == 0 and lo["rows"] == 0, (Kp, F, m, lo)  # every wavefront's base is 16-byte aligned
        assert lo["per_wave"] == K.per_wave_bytes(Kp, F, m), (Kp, F, m, lo)


# ---------------------------------------------------------------- refresh and grids over the batches of the existing cases
def plan_batches(X, batch, solver, perms=None):
    """[(first_singleton, b, sample ids, stored)]: K.fit_batches with the plan's view of every batch beside it"""
    out = []
    for e in range(K.EPOCHS):
        order = np.arange(X.n) if perms is None else np.asarray(perms[e])
        first = solver == "adagrad" and e == 0
        out += [(first, b, order[lo:hi], first and b == 0) for b, (lo, hi) in enumerate(K.batches(X.n, batch, first))]
    want = K.fit_batches(X.n, batch, solver, perms)
    assert len(out) == len(want) and all(o[3] == w[1] and np.array_equal(o[2], w[0]) for o, w in zip(out, want))
    return out


def batch_numbers(X, ids, b):
    c = K.batch_counts(X, ids)
    heavy = c[c > K.kHeavyTouches]
    return Batch(b, len(ids), int(np.count_nonzero(c)), int(c.sum()), len(heavy), int((-(-heavy // K.kHeavySegment)).sum()))


@functools.lru_cache(maxsize=None)
def data_sets():
    """(name, X, batch, perms, k of its row kernel or None) of the refresh regimes, the column data and three row cases"""
    out = [("refresh_" + r, K.refresh_data(r)[0], K.COL_BATCH, None) for r in K.REFRESH]
    out += [("col_%d" % c, K.col_data(bool(c))[0], K.COL_BATCH, None) for c in (0, 1)]
    out += [(n, K.row_data(n)[0], K.BATCH, K.row_perms()) for n in K.FLAG_CASES]
    return out


def test_refresh_is_the_restatements_per_batch():
    seen = set()
    for name, X, batch, perms in data_sets():
        for solver, opt in (("sgd", SGD), ("adagrad", ADAGRAD)):
            plan = plan_batches(X, batch, solver, perms)
            S = [Shape(1, opt, X.F, 2, int(X.lengths().max()), int(first)) for first, _, _, _ in plan]
            B = [batch_numbers(X, ids, b) for _, b, ids, _ in plan]
            for knob in (None, 0, 2):
                got = run([line(s, Knobs(refresh=knob), bb) for s, bb in zip(S, B)])
                for (first, b, ids, stored), bb, g in zip(plan, B, got):
                    want = solver == "adagrad" and not stored and knob != 0 and (knob == 2 or bb.touches >= 4 * bb.uniq)
                    assert g["refresh"] == int(want) and g["use_stored"] == int(stored or want), (name, solver, knob, b)
                    assert (g["nR"] > 0) == want and g["off_refresh"] == 0, (name, solver, knob, b)
                    seen.add((name, solver, knob, bool(want)))
                if knob is None:
                    assert sum(g["refresh"] for g in got) == K.refresh_batches(X, batch, solver, perms), (name, solver)
                if knob == 2 and solver == "adagrad":  # everything but the stored first step
                    assert [g["refresh"] for g in got] == [int(not stored) for _, _, _, stored in plan], name
    assert not any(want for _, solver, knob, want in seen if solver == "sgd" or knob == 0)
    assert ("refresh_dense", "adagrad", None, True) in seen and ("refresh_sparse", "adagrad", None, False) in seen
    assert ("refresh_sparse", "adagrad", 2, True) in seen and ("col_0", "adagrad", None, True) in seen


def ceil_div(a, b):
    return -(-a // b)


def grids(L, F, wpb, B, refresh):
    """the five grids as the issue states them: R = 64 / L lane groups per wavefront, 4 wavefronts per workgroup"""
    R = 64 // L
    units = ceil_div(B.uniq * F, 4 * R)
    return {"nA": ceil_div(B.len, wpb), "nR": max(1, units) if refresh else 0, "nB": units + 1, "nsb": ceil_div(B.segs * F, 4 * R),
            "nH": ceil_div(B.heavy * F, 4)}


def check_grids(g, L, F, B, what):
    want = grids(L, F, g["wpb"], B, g["refresh"])
    assert {k: g[k] for k in want} == want, (what, g, want)
    assert (g["off_refresh"], g["off_col"], g["off_heavy"]) == (0, g["nR"], g["nR"] + g["nB"]), what
    assert g["n_parts"] == g["nR"] + g["nB"] + g["nH"], what


def test_the_grids_of_every_batch_at_every_lane_width():
    seen = {"heavy": set(), "kernel": set(), "refresh": set()}
    n_heavy = {}
    for name, X, batch, perms in data_sets():
        for solver, opt in (("sgd", SGD), ("adagrad", ADAGRAD)):
            plan = plan_batches(X, batch, solver, perms)
            B = [batch_numbers(X, ids, b) for _, b, ids, _ in plan]
            n_heavy[name, solver] = (sum(bb.heavy > 0 for bb in B), max(-(-int(K.batch_counts(X, ids).max()) // K.kHeavySegment) if bb.heavy else 0
                                                                       for (_, _, ids, _), bb in zip(plan, B)))
            for L in LS:
                S = [Shape(L, opt, X.F, 2 * L, int(X.lengths().max()), int(first)) for first, _, _, _ in plan]
                for s, bb, g in zip(S, B, run([line(s, Knobs(), bb) for s, bb in zip(S, B)])):
                    assert g["wpb"] == (1 if K.row_kernel(2 * L, X.F, s.max_row)[0] == "coop" else 4)
                    check_grids(g, L, X.F, bb, (name, solver, L, bb))
                    assert (g["nH"] > 0) == (g["nsb"] > 0) == (bb.heavy > 0)
                    seen["heavy"].add(bb.heavy > 0)
                    seen["kernel"].add(g["kernel"])
                    seen["refresh"].add(bool(g["refresh"]))
            if perms is None:  # the heavy batches as tests/ffm_kernel_cases.py counts them
                assert n_heavy[name, solver] == K.heavy_batches(X, batch, solver), (name, solver)
    assert seen["heavy"] == seen["refresh"] == {False, True} and seen["kernel"] == set(KERNELS)
    assert n_heavy["col_0", "sgd"] == (6, 3) and n_heavy["col_1", "sgd"] == (0, 0)


# ---------------------------------------------------------------- the bounds
def old_bounds(F, Kp, M):
    """what mb_ffm_epoch asked for before ffm_work_bounds (its own formulas, integer divisions as they stood)"""
    return {"contrib": max(M.touch, 1) * F * Kp, "rec": max(M.batch, 1), "partsA": M.batch + 1,
            "partsB": 2 * (2 * (M.unique * F // 4) + M.heavy * F // 4 + 8), "hpart": max(M.segs, 1) * F * (2 * Kp + 4)}


@functools.lru_cache(maxsize=None)
def draws(n=6000):
    """seeded: a shape under each of the three row kernels, both optimizers, the refresh knob unset / 0 / 2, a plan's maxima and a
    batch within them -- every third one at the maxima themselves"""
    rng = np.random.default_rng(20)
    rows = {"generic": lambda L: (int(rng.integers(1, 70)), 65 + int(rng.integers(0, 3))),  # (F, max_row)
            "lds": lambda L: (int(rng.integers(1, 4)), int(rng.integers(0, 6))),
            "coop": lambda L: ((64, 64) if L == 1 else (40, 40) if L <= 4 else (128 // L, 40))}  # from L = 8 on: 80 KiB of rows
    cs = []
    for i in range(n):
        L, want = int(rng.choice(LS)), KERNELS[i % 3]
        F, max_row = rows[want](L)
        assert K.row_kernel(2 * L, F, max_row)[0] == want, (L, F, max_row, want)
        S = Shape(L, int(rng.integers(0, 2)), F, 2 * L, max_row, int(rng.integers(0, 2)))
        Kn = Knobs(None, (None, 0, 2)[int(rng.integers(0, 3))])
        mh = int(rng.integers(0, 4)) * int(rng.integers(0, 2))
        M = Maxima(int(rng.integers(0, 3000)), int(rng.integers(0, 2000)), int(rng.integers(0, 50000)), mh, mh * int(rng.integers(3, 8)))
        if i % 3 == 0:
            B = Batch(int(rng.integers(0, 3)), *M)
        else:
            heavy = int(rng.integers(0, M.heavy + 1))
            B = Batch(int(rng.integers(0, 3)), int(rng.integers(0, M.batch + 1)), int(rng.integers(0, M.unique + 1)), int(rng.integers(0, M.touch + 1)),
                      heavy, int(rng.integers(heavy, M.segs + 1)) if heavy else 0)
        cs.append((S, Kn, B, M))
    return cs, run([line(*c) for c in cs])


def test_the_bounds_hold_every_route_and_stay_within_the_old_ones():
    cs, got = draws()
    tight = collections.Counter()
    for (S, Kn, B, M), g in zip(cs, got):
        b, old = g["bounds"], old_bounds(S.nb, S.Kp, M)
        check_grids(g, S.L, S.nb, B, (S, Kn, B))
        assert g["nA"] <= b["partsA"] and g["n_parts"] <= b["partsB"] // 2 and b["partsB"] % 2 == 0, (S, Kn, B, M, g)
        assert B.len <= b["rec"] and B.touches * S.nb * S.Kp <= b["contrib"] and B.segs * S.nb * (2 * S.Kp + 4) <= b["hpart"], (S, Kn, B, M, g)
        assert 0 < b["partsA"] <= old["partsA"] and 0 < b["partsB"] <= old["partsB"], (S, M, b, old)
        assert (b["contrib"], b["hpart"], b["rec"]) == (old["contrib"], old["hpart"], old["rec"]), (S, M, b, old)
        tight["partsA"] += g["nA"] == b["partsA"]
        tight["partsB"] += g["n_parts"] == b["partsB"] // 2
        tight[g["kernel"], bool(g["refresh"])] += 1
    assert tight["partsA"] > 100 and tight["partsB"] > 100  # the bounds are reached, not merely large
    assert all(tight[kn, r] > 100 for kn in KERNELS for r in (False, True))


# ---------------------------------------------------------------- the knobs; the sanitizers
def test_the_knobs_are_read_from_the_environment():
    env = {k: v for k, v in os.environ.items() if k not in ("NFM_FFM_LDS", "NFM_FFM_REFRESH")}
    for lds, refresh in ((None, None), ("0", "2"), ("1", "0"), ("", "x")):
        e = dict(env, **{k: v for k, v in (("NFM_FFM_LDS", lds), ("NFM_FFM_REFRESH", refresh)) if v is not None})
        out = subprocess.run([exe(), "knobs"], capture_output=True, text=True, timeout=60, env=e)
        want = [UNSET if v is None else int(v) if v.isdigit() else 0 for v in (lds, refresh)]  # atoi
        assert out.returncode == 0 and [int(v) for v in out.stdout.split()] == want, (lds, refresh, out.stdout)


def test_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined, on every fifth draw and every 31st case of the grid: no report (a
    report ends it with a nonzero status), the same answers"""
    lines = [line(*c) for c in draws()[0][::5]] + [line(Shape(Kp // 2, ADAGRAD, F, Kp, m, 1), Knobs(), ONE) for Kp, F, m in grid()[0][::31]]
    assert run(lines, sanitize=True) == run(lines)
