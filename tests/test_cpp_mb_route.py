"""The route of a mini-batch (nimfm_amd/csrc/mb_route.h: which row and column kernel, what is staged, every grid size, the work
buffers' bounds) is plain C++: tests/cpp/mb_route_test.cpp builds with g++ alone -- no HIP, no library -- reads cases on stdin and
prints the header's answers.  They are held against the two restatements: tests/row_slot_cases.py (the row phase of every case of
its table, both epochs, every batch) and tests/mb_route_cases.py (column kernel, staging, grids, over draws from the grid of
thresholds), and the bounds against the routes they must hold.  Built the way tests/test_cpp_seqwin_layout.py builds its program;
a second build with -fsanitize=address,undefined runs the same input stand-alone."""
import functools
import os
import subprocess

import mb_route_cases as C
import row_slot_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mb_route_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_mb_route_test")


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def run(lines, sanitize=False):
    env = {k: v for k, v in os.environ.items() if k != "NFM_SPLIT"}
    out = subprocess.run([exe(sanitize)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) and "%d cases" % len(lines) in out.stderr
    return got


# ---------------------------------------------------------------- the row phase against tests/row_slot_cases.py
def row_case_lines():
    """[(case, Path, input line)] for every batch of both epochs of every case of the table, under NFM_STAGE_W=1"""
    out = []
    for c in R.table():
        X, _ = R.train_data(c.family, c.regime)
        d, batch = R.REGIMES[c.regime]
        degree, fit_lower, fit_linear = R.MODELS[c.model]
        nb, n_aug = R.n_orders(degree, fit_lower), R.n_augments(degree, fit_lower, fit_linear)
        opt = {"sgd": C.SGD, "adagrad": C.ADAGRAD, "mbpsgd": C.PSGD}[c.solver]
        for p in R.fit_paths(c):
            S = C.Shape(p.L, opt, int(p.gen), nb, n_aug, int(fit_linear), d, int(X.lengths().max()), len(X.data) / X.n + n_aug, 256,
                        int(p.singles), int(p.first), 0, 8 * nb * (d + n_aug) * 2 * p.L, 1, 5)
            B = C.Batch(p.b, p.samples, 1, 1, 0, 0)
            out.append((c, p, C.line(c.request, S, C.Knobs(stage_w=1), B)))
    return out


def test_the_row_phase_is_the_restatements():
    rows = row_case_lines()
    assert len(rows) > 1000
    got = [C.parse(ln) for ln in run([ln for _, _, ln in rows])]
    staged = {}
    for (c, p, _), g in zip(rows, got):
        key = (c, p.b, p.first)
        assert g["use_stored"] == p.stored, key
        assert (g["held"], g["cap"]) == (R.held_entries(p.L, g["slots"]), R.held_capacity(p.L, g["slots"])), key
        if p.kernel == "ada2":
            assert (g["row"], g["slots"], g["nA"], g["counters"][0]) == ("ada2", 2, (p.samples + 1) // 2, "route_row_ada2"), key
            continue
        assert (g["row"], g["slots"], g["mode"], g["sing"]) == ("row", p.slots, p.mode, p.sing), (key, g)
        assert (g["held"], g["cap"]) == (p.held, p.cap) and g["counters"][0] == "route_row_m%d" % p.mode, key
        assert g["nA"] == -(-p.samples // (4 * (64 // (p.L * p.slots)))), key
        staged.setdefault(c, g["w_cap"] if g["stage_w"] != "gather" else 0)  # the first batch of the fit, as stage_w_cap
        assert g["stage_w"] != "ranges"  # rows that do not all ascend: slices
    for c in R.table():
        if c in staged:
            assert staged[c] == R.stage_w_cap(c), c
    assert set(staged.values()) == {0, 32, 64}


# ---------------------------------------------------------------- column kernel, staging, grids, bounds
@functools.lru_cache(maxsize=None)
def grid():
    cs = C.cases()
    return cs, [C.parse(ln) for ln in run([C.line(0, *c) for c in cs])]


COMPARED = ("use_stored", "row", "slots", "mode", "sing", "stream_rows", "nA", "singles_in_row", "singles_in_col", "nS", "stage_w", "w_cap", "w_parts",
            "w_wg", "w_slice", "stage_dl", "dl_grid", "col", "nB", "nsb", "nH")


def test_every_choice_and_grid_is_the_restatements():
    cs, got = grid()
    seen = {k: set() for k in ("col", "row_mode", "stage_w", "stage_dl", "bad", "capped", "stream", "nS", "nH", "parts")}
    for (S, K, B), g in zip(cs, got):
        want = C.route(S, K, B)
        assert g["bad_passes"] == want["bad_passes"], (S, K, B)
        seen["bad"].add((want["bad_passes"], K.stage_w_passes, want["w_cap"]))
        if want["bad_passes"]:
            continue
        assert {k: g[k] for k in COMPARED} == {k: want[k] for k in COMPARED}, (S, K, B, g, want)
        assert g["counters"] == ("route_row_ada2" if g["row"] == "ada2" else "route_row_m%d" % g["mode"], "route_col_" + g["col"])
        seen["col"].add((g["col"], all(v is None for v in K)))
        seen["row_mode"].add((g["row"], g["mode"], g["sing"]))
        seen["stage_w"].add((g["stage_w"], g["w_cap"], g["w_parts"] > 1))
        seen["stage_dl"].add(g["stage_dl"])
        seen["stream"].add(g["stream_rows"])
        seen["nS"].add(g["nS"] > 0)
        seen["nH"].add(g["nH"] > 0)
    # what the draw reached: every kernel (those without a tuning variant with every knob unset too), every row mode, both staging
    # kernels at both strides with one and with several slices / passes, the refusals the issue names
    assert {c for c, _ in seen["col"]} == set(C.COL_KERNELS)
    assert {c for c, dflt in seen["col"] if dflt} == {"phase", "strided", "sparse", "long", "long_compact"}
    assert seen["row_mode"] >= {("row", 0, False), ("row", 0, True), ("row", 1, False), ("row", 2, False), ("row", 3, False), ("row", 4, False),
                                ("ada2", 0, False)}
    assert seen["stage_w"] >= {(k, cap, many) for k in ("slices", "ranges") for cap in (32, 64) for many in (False, True)}
    assert seen["stage_dl"] == seen["stream"] == seen["nS"] == seen["nH"] == {False, True}
    assert (True, 3, 32) in seen["bad"] and (True, 3, 64) in seen["bad"] and (True, 64, 32) in seen["bad"] and (False, 64, 64) in seen["bad"]
    assert not any(bad for bad, passes, _ in seen["bad"] if passes in (None, 0, 1, 4))
    # every value of every axis of the grid
    for f in C.Shape._fields:
        assert len({getattr(S, f) for S, _, _ in cs}) >= 2, f
    assert {S.L for S, _, _ in cs} == {1, 2, 4, 8, 16, 32, 64} and {S.max_row + S.n_aug for S, _, _ in cs} == set(C.WIDEST)
    assert {B.len for _, _, B in cs} == set(C.LENS)
    for k, vals in C.KNOB_VALUES.items():
        assert {getattr(K, k) for _, K, _ in cs} == set(vals), k


def test_the_bounds_hold_every_route():
    """with the batch's own numbers as the plan's maxima: every workgroup has its partial, every staged stream its buffer -- so no
    batch is left unstaged for want of a buffer, the route does not look at them"""
    cs, got = grid()
    tight = {"partsA": 0, "partsB": 0}
    for (S, K, B), g in zip(cs, got):
        if g["bad_passes"]:
            continue
        b = g["bounds"]
        assert g["nA"] <= b["partsA"], (S, K, B, g)
        assert g["nS"] + g["nB"] + g["nH"] <= b["partsB"] // 2 and b["partsB"] % 2 == 0, (S, K, B, g)
        if g["stage_w"] != "gather":
            assert b["Wt"] >= B.len * g["w_cap"] > 0, (S, K, B, g)
        if g["stage_dl"]:
            assert b["dLt"] >= B.touches > 0, (S, K, B, g)
        tight["partsA"] += g["nA"] == b["partsA"]
        tight["partsB"] += g["nS"] + g["nB"] + g["nH"] == b["partsB"] // 2
    assert tight["partsA"] > 0 and tight["partsB"] > 0  # the bounds are reached, not merely large


def test_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined, on every fifth case of the grid and every seventh row case: no
    report (a report ends it with a nonzero status), the same answers"""
    lines = [C.line(0, *c) for c in grid()[0][::5]] + [ln for _, _, ln in row_case_lines()[::7]]
    assert run(lines, sanitize=True) == run(lines)
