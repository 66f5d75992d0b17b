"""The routes of a sequential-mode call (nimfm_amd/csrc/seq_route.h: the window's view, support, offer, flavour, worker, worker
count, LDS bytes and buffer counts; the one-workgroup kernels' step, threads, rows per thread, LDS bytes and table placement) are
plain C++: tests/cpp/seq_route_test.cpp builds with g++ alone -- no HIP, no library -- reads cases on stdin and prints the header's
answers.  They are held, field by field, against the restatement of tests/seq_route_cases.py over its grids, against properties
every launch must have, and -- inside the program -- against a copy of the lines the header replaced, over seeded random draws.
Built the way tests/test_cpp_mb_ffm_route.py builds its program; a second build with -fsanitize=address,undefined runs stand-alone."""
import collections
import functools
import os
import re
import subprocess

import seq_route_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seq_route_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_seq_route_test")
CSRC = os.path.join(ROOT, "nimfm_amd", "csrc")
UNSET = -2147483648
KIB160 = 160 * 1024

WIN_INTS = ("two_block nb Kp supported reason offered no_cond one_term worker W lgW first_worker m_cap lgKp terms ch FW np thr near_r par_min "
            "lds_worker lds_cond lds_bytes n_fwd n_res n_ctl n_partial n_fw n_fw_tags n_scales fits_cus fits").split()
ONE_INTS = "refusal step m_cap T threads S lgS rc split_terms lds_bytes table_in_lds table_bytes".split()


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def line(S, K, fallbacks=0, snap_bytes=0):
    return " ".join(str(int(UNSET if v is None else v)) for v in tuple(S) + tuple(K) + (fallbacks, snap_bytes))


def parse(ln):
    win, one = (part.split() for part in ln.split("|"))
    w = dict(zip(WIN_INTS, map(int, win[:-1])))
    w["reason"], w["worker"], w["counter"] = C.REASONS[w["reason"]], C.WORKERS[w["worker"]], win[-1]
    o = dict(zip(ONE_INTS, map(int, one[:-1])))
    o["refusal"], o["step"], o["counter"] = C.REFUSALS[o["refusal"]], C.STEPS[o["step"]], one[-1]
    return w, o


def run(lines, sanitize=False):
    out = subprocess.run([exe(sanitize)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) and "%d cases" % len(lines) in out.stderr
    return [parse(ln) for ln in got]


@functools.lru_cache(maxsize=None)
def window():
    cs = C.window_cases()
    return cs, [g[0] for g in run([line(S, K, fb, snap) for _, S, K, fb, snap in cs])]


@functools.lru_cache(maxsize=None)
def one_wg():
    cs = C.one_wg_cases()
    return cs, [g[1] for g in run([line(S, K) for _, S, K in cs])]


# ---------------------------------------------------------------- the window
def test_the_window_route_of_every_case_is_the_restatements():
    cs, got = window()
    seen = collections.Counter()
    for (name, S, K, fb, snap), g in zip(cs, got):
        want = C.win_route(S, K, fb, snap)
        assert {k: g[k] for k in want} == want, (name, S, K, fb, snap, {k: (g[k], v) for k, v in want.items() if g[k] != v})
        if not want["supported"]:  # nothing of a launch is set
            assert g["counter"] == "-" and g["W"] == g["lds_bytes"] == g["fits"] == 0, (name, S, K)
        seen[want["reason"]] += 1
        seen[want.get("worker"), want["no_cond"], want["one_term"]] += 1
        seen["two_block", want["two_block"], want["supported"]] += 1
        seen["offered", want["offered"]] += 1
        seen["fits", want.get("fits_cus"), want.get("fits")] += 1
        seen["W", want.get("W")] += 1
    assert len(cs) > 50000
    assert all(seen[r] > 0 for r in C.REASONS), seen
    for wk in C.WORKERS:  # every worker without a conductor, with the one-term chain and term by term
        assert all(seen[wk, nc, ot] > 0 for nc, ot in ((1, 0), (0, 1), (0, 0))), (wk, seen)
    assert all(seen["two_block", tb, s] > 0 for tb in (0, 1) for s in (0, 1))
    assert seen["offered", 0] > 0 and seen["offered", 1] > 0
    # (17 CUs hold the smallest window, so a supported route always fits the CUs; (1, 0): offered, then refused for its LDS)
    assert seen["fits", 1, 1] > 0 and seen["fits", 0, 0] == 0 and seen["fits", 1, 0] > 0
    assert all(seen["W", W] > 0 for W in (16, 32, 64, 128, 256))


def test_every_supported_and_fitting_window_route_can_be_launched():
    cs, got = window()
    n = 0
    for (name, S, K, fb, snap), g in zip(cs, got):
        assert g["offered"] <= g["supported"] and g["fits"] <= g["fits_cus"] <= g["supported"], (name, S, K)
        if not (g["supported"] and g["fits"]):
            continue
        n += 1
        what = (name, S, K, fb, g)
        assert C.LDS_FLOOR <= g["lds_bytes"] <= KIB160 and g["lds_bytes"] >= max(g["lds_worker"], g["lds_cond"]), what
        assert g["W"] == 1 << g["lgW"] and 16 <= g["W"] <= 256, what
        assert g["W"] + g["first_worker"] <= S.n_cu and g["first_worker"] == 1 - g["no_cond"], what
        assert g["W"] > C.WIN_DEPTH, what
        assert g["ch"] in (32, 64) and g["FW"] > C.WIN_HDR and (g["FW"] - C.WIN_HDR) % g["ch"] == 0, what
        assert g["one_term"] or g["FW"] - C.WIN_HDR >= g["terms"], what  # a term-by-term mailbox holds every term,
        assert g["one_term"] or g["no_cond"] or g["FW"] <= 64 * C.WIN_MAX_NL, what  # ... in the loads the conductor's fetch makes
        assert g["n_fwd"] >= (C.SUM_GRAN * g["np"] * g["W"] if g["one_term"] else g["W"] * g["np"] * g["FW"]), what
        assert g["n_res"] >= g["W"] * g["np"] * C.RES_WORDS and g["n_ctl"] > g["W"] and g["n_partial"] >= 2 * (g["W"] + g["first_worker"]), what
        assert g["n_fw"] >= g["n_fw_tags"] >= C.FW_SLOT * g["np"] * g["W"] and g["n_scales"] == (0 if S.ada else 2 * S.ns), what
        assert g["np"] in (2, 4) and g["thr"] * g["W"] + g["near_r"] <= g["np"] * g["W"], what  # (WinArgs::thr)
        assert not g["one_term"] or (not g["no_cond"] and C.SUM_RING >= 2 * g["W"]), what
        assert g["counter"] == "seq_route_win_" + g["worker"] and 2 <= g["Kp"] <= 64 and 1 << g["lgKp"] == g["Kp"], what
    assert n > 20000


def test_the_w_8_of_the_gpu_tests_is_sixteen_workers():
    """the launcher's floor: NFM_SEQ_WIN_W below 16 is 16 workers (tests/test_gpu_seqwin.py's W = 8 ids run 16)"""
    for _, S in C.worker_models():
        for w in (1, 8, 15, 16, 31):
            assert C.win_route(S, C.Knobs(win=2, w=w))["W"] == (16 if w < 32 else 32)
    got = run([line(S, C.Knobs(win=2, w=8)) for _, S in C.worker_models()])
    assert {g[0]["W"] for g in got} == {16}


# ---------------------------------------------------------------- one workgroup
def test_the_one_workgroup_route_of_every_case_is_the_restatements():
    cs, got = one_wg()
    seen = collections.Counter()
    for (name, S, K), g in zip(cs, got):
        want = C.one_wg_route(S, K)
        assert {k: g[k] for k in want} == want, (name, S, K, {k: (g[k], v) for k, v in want.items() if g[k] != v})
        if want["refusal"] != "ok":
            assert g["counter"] == "-" and g["T"] == g["lds_bytes"] == 0
            seen[want["refusal"]] += 1
            continue
        seen[want["counter"]] += 1
        seen[want["step"], want["threads"], want["rc"]] += 1
        seen["split", want["step"], want["split_terms"]] += 1
    assert all(seen[c] > 0 for c in ("seq_route_pipe", "seq_route_pipe_wide", "seq_route_staged", "seq_route_plain", "seq_route_plain_scratch", "kp", "degree"))
    # every rung that can be chosen: 9 ... 32 rows per thread of 256 always halve at 512 threads, and 512 are taken from 8 rows per
    # thread of 256 on, i.e. at least 4 of 512 -- so <.., 16, 256>, <.., 32, 256> and <.., 2, 512> are instantiated and never launched
    assert {k[1:] for k in seen if k[0] == "pipe"} == {(256, rc) for rc in (1, 2, 4, 8, 64)} | {(512, rc) for rc in (4, 8, 16)}, seen
    assert seen["split", "pipe", 0] > 0 and seen["split", "pipe", 1] > 0


def test_every_one_workgroup_route_can_be_launched():
    cs, got = one_wg()
    for (name, S, K), g in zip(cs, got):
        if g["refusal"] != "ok":
            continue
        what = (name, S, K, g)
        if g["step"] == "pipe":
            assert g["rc"] in ((2, 4, 8, 16) if g["threads"] == 512 else (1, 2, 4, 8, 16, 32, 64)) and g["threads"] in (256, 512), what
            G = g["threads"] // g["S"]
            slots = (S.nb if S.kind == C.FFM else 1) * g["m_cap"]
            assert g["S"] == 1 << g["lgS"] and g["S"] >= S.Kp and G >= 1 and g["rc"] * G >= slots, what  # RC * G >= rows per sample
        else:
            assert g["threads"] == g["T"] and g["T"] % 64 == 0 and g["T"] >= max(S.Kp, 64), what
            assert g["table_bytes"] == 8 * max(S.nb, 1) * g["m_cap"] * g["T"], what
            assert g["step"] == "plain" or g["table_in_lds"], what
        if g["table_in_lds"]:
            assert g["lds_bytes"] <= KIB160 and g["lds_bytes"] >= 8 * g["threads"] + (g["table_bytes"] if g["step"] != "pipe" else 0), what
        else:
            assert g["lds_bytes"] == 8 * g["T"] and 8 * g["T"] + g["table_bytes"] > KIB160 and g["counter"] == "seq_route_plain_scratch", what


def test_the_edges_of_the_one_workgroup_route():
    """one row either side of each 160 KiB edge and of each threshold the issue names, by the restatement and by the header"""
    def at(Kp, m, nb=1, kind=C.FM, **knobs):
        S = C.Shape(kind, 2 if nb == 1 or kind == C.FFM else 3, nb, 1, Kp, Kp, 0, 1, 1000, 1000, 1 if kind == C.FFM else 1000, nb if kind == C.FFM else 1, m,
                    4096, 4096 * m, 0, 256)
        return S, C.Knobs(**knobs)
    cases = {
        "table_last_in_lds": (at(64, 319, pipe=0), ("plain", 1)), "table_first_in_scratch": (at(64, 320, pipe=0), ("plain", 0)),
        "staged_last": (at(64, 155, pipe=0), ("staged", 1)), "staged_first_plain": (at(64, 156, pipe=0), ("plain", 1)),
        "pipe_m256": (at(8, 256), ("pipe", 1)), "pipe_m257": (at(8, 257), ("plain", 1)),
        "pipe_rows_7_per_thread": (at(64, 28), ("pipe", 1)), "pipe_rows_8_go_wide": (at(64, 29), ("pipe", 1)),
        "pair_table_m64": (at(8, 64, nb=2, kind=C.FFM), ("pipe", 1)), "pair_table_m65": (at(8, 65, nb=2, kind=C.FFM), ("pipe", 1)),
        "kp_1024": (at(1024, 4), ("staged", 1)), "kp_1025": (at(1025, 4), None),
    }
    got = run([line(*c[0]) for c in cases.values()])
    for (name, ((S, K), want)), (_, g) in zip(cases.items(), got):
        r = C.one_wg_route(S, K)
        assert {k: g[k] for k in r} == r, name
        assert (None if g["refusal"] != "ok" else (g["step"], g["table_in_lds"])) == want, (name, g)
    by = dict(zip(cases, (g[1] for g in got)))
    assert by["pipe_rows_7_per_thread"]["threads"] == 256 and by["pipe_rows_8_go_wide"]["threads"] == 512
    assert by["pipe_rows_7_per_thread"]["rc"] == 8 and by["pipe_rows_8_go_wide"]["rc"] == 4
    assert by["pair_table_m65"]["lds_bytes"] - by["pair_table_m64"]["lds_bytes"] < 8 * 64 * 64  # no pair table beyond the cap
    assert by["kp_1025"]["refusal"] == "kp"
    # split_terms: the widest pipelined rows lose their table of terms first
    walk = [C.one_wg_route(*at(256, m)) for m in range(1, 60)]
    assert {(r["step"], r["split_terms"]) for r in walk} >= {("pipe", 1), ("pipe", 0)}


# ---------------------------------------------------------------- the parent's lines; the knobs; the sources; the sanitizers
def test_the_header_against_the_lines_it_replaced():
    out = subprocess.run([exe(), "parent", "12000", "7"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if not k.startswith("NFM_SEQ_")})
    assert out.returncode == 0 and "DISAGREE" not in out.stdout, out.stdout[-4000:]
    m = re.search(r"draws (\d+) disagreements (\d+) \| supported (\d+) offered (\d+) refused_cus (\d+) refused_lds (\d+) two_block (\d+) \| "
                  r"pipe (\d+) staged (\d+) scratch (\d+)", out.stdout)
    n = [int(v) for v in m.groups()]
    assert n[0] == 12000 >= 6000 and n[1] == 0
    assert min(n[2:4]) > 500 and n[6] > 50 and min(n[7:]) > 300, out.stdout  # the draws reach what they compare
    assert n[5] > 0, out.stdout  # the corner kept: a call the window is offered and its launcher refuses (NFM_SEQ_WIN_W, LDS)


KNOBS = ("NFM_SEQ_WIN", "NFM_SEQ_WIN_EXACT", "NFM_SEQ_WIN_NOCOND", "NFM_SEQ_WIN_W", "NFM_SEQ_WIN_PAR", "NFM_SEQ_WIN_TRACE", "NFM_SEQ_PIPE",
         "NFM_SEQ_STAGE", "NFM_SEQ_WIN_TRACE_FILE")


def test_the_knobs_are_read_from_the_environment():
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    for vals in ((None,) * 9, ("2", "1", "0", "8", "0", "1", "0", "0", "/tmp/t.bin"), ("0", "0", "1", "1000", "9", "0", "1", "1", None),
                 ("", "x", "2", "-4", "6", "", "x", "", "")):
        e = dict(env, **{k: v for k, v in zip(KNOBS, vals) if v is not None})
        out = subprocess.run([exe(), "knobs"], capture_output=True, text=True, timeout=60, env=e)
        want = [UNSET if v is None else int(v) if re.fullmatch(r"-?\d+", v) else 0 for v in vals[:8]]  # atoi
        got = out.stdout.split(" ", 8)
        assert out.returncode == 0 and [int(v) for v in got[:8]] == want, (vals, out.stdout)
        assert got[8].rstrip("\n") == ("-" if vals[8] is None else vals[8]), (vals, out.stdout)


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def outside_test_hooks(text):
    return re.sub(r"#ifdef NFM_TEST_HOOKS.*?#endif", "", text, flags=re.S)


def test_the_source_still_has_the_choices_restated():
    """the header is the one reader of the driver's environment, and the sources it took the decisions from call it"""
    route, seqwin, seq, api, step = (src(f) for f in ("seq_route.h", "seqwin.hip", "seq.hip", "api.hip", "seq_step.h"))
    for text in (seqwin, seq, step):
        assert "getenv" not in outside_test_hooks(text)
    assert "NFM_SEQ_WIN_TEST_DEAD_SLOT" in seqwin and "NFM_TEST_NO_SNAPSHOT" in api  # the two hooks stay where they act ...
    assert "NFM_SEQ_" not in outside_test_hooks(api) and "DEAD_SLOT" not in route and "NO_SNAPSHOT" not in route  # ... and nowhere else
    sequential = api[api.index("// -- NFM_MODE_SEQUENTIAL --"):api.index("// -- NFM_MODE_MINIBATCH --")]
    assert "getenv" not in outside_test_hooks(sequential)
    assert sequential.count("win_route(") == 1 and sequential.count("seq_knobs()") == 1
    assert route.count("getenv(") == 1 and all('"%s"' % k in route for k in KNOBS)  # (the file name; the rest through mb_knob)
    assert "const SeqOneWg r = seq_one_wg_route(" in seq
    for gone in ("seq_window_supported", "win_no_cond", "win_one_term", "win_worker_lds", "win_ffm_terms"):
        assert gone not in seqwin + api + src("opt_views.h")
    assert "static_assert(SEQ_KIND_FM == NFM_KIND_FM && SEQ_KIND_FFM == NFM_KIND_FFM" in src("opt_views.h")
    assert "static_assert(kWinLdsWave == kWave && kWinLdsMaxDeg == dev::kMaxDeg" in seqwin
    # the constants the restatement carries
    for text in ("kWinRing = 8;", "kWinDepth = 8;", "kWinHdr = 4;", "kWinMaxNL = 5;", "kSumGran = 13;", "kSumRing = 256;", "kResWords = 4;",
                 "kSeqMaxDeg = 8;", "kPipeThreads = 256;", "kPipeThreadsWide = 512;", "kPipePairCap = 4096;", "kWinLdsFloor = 81 * 1024;",
                 "kSeqLdsMax = 160 * 1024;", "0.8e-6 * 0.25", "2.0e12"):
        assert text in route, text


def test_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined, on every 23rd window case, every 11th one-workgroup case and 2000
    draws against the parent's lines: no report (a report ends it with a nonzero status), the same answers"""
    wc, oc = C.window_cases()[::23], C.one_wg_cases()[::11]
    lines = [line(S, K, fb, snap) for _, S, K, fb, snap in wc] + [line(S, K) for _, S, K in oc]
    assert run(lines, sanitize=True) == run(lines)
    env = {k: v for k, v in os.environ.items() if not k.startswith("NFM_SEQ_")}
    a = subprocess.run([exe(True), "parent", "2000", "3"], capture_output=True, text=True, timeout=600, env=env)
    b = subprocess.run([exe(), "parent", "2000", "3"], capture_output=True, text=True, timeout=600, env=env)
    assert a.returncode == 0 and a.stdout == b.stdout and "disagreements 0" in a.stdout, a.stdout[-2000:] + a.stderr[-4000:]
