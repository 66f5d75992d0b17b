"""The route of a batch-plan build (nimfm_amd/csrc/plan_route.h: batch bounds, the width of the sort's key, whether the column-major
twin and bucketing are tried and in which instantiation, the rungs, the count-order key) is plain C++:
tests/cpp/plan_route_test.cpp builds with g++ alone -- no HIP, no library -- reads cases on stdin and prints the header's answers.
They are held, field by field, against the restatement of tests/plan_route_cases.py over its grids, against properties every answer
must have, and -- inside the program -- against a copy of the lines the header replaced, over seeded random draws.  Built the way
tests/test_cpp_seq_route.py builds its program; a second build with -fsanitize=address,undefined runs stand-alone."""
import collections
import functools
import os
import re
import subprocess

import plan_route_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plan_route_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_plan_route_test")
CSRC = os.path.join(ROOT, "nimfm_amd", "csrc")
UNSET = -2147483648
BUILDERS = ("sort", "twin", "seg")  # Plan::kBySort, kByTwin, kBySeg

TWIN_INTS = "wanted build_first by_key tried ne wpb per_wave lds_bytes clashed".split()
SEG_INTS = "consulted tried fl nbk cells S cpb pbits qbits narrow sh_pos sh_fl qmask pmask xcd gives_up ipt fill_lds".split()


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    out = EXE + ("_san" if sanitize else "")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", out])
    return out


def run(lines, sanitize=False):
    out = subprocess.run([exe(sanitize)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) and "%d cases" % len(lines) in out.stderr
    return got


def route_line(S, K, T, clash, touches, h_mx):
    vals = tuple(S) + tuple(UNSET if v is None else v for v in K) + (T, clash, -1 if touches is None else touches, h_mx)
    return "R " + " ".join(str(int(v)) for v in vals)


def parse_route(ln):
    rng, tw, sg, end = (part.split() for part in ln.split("|"))
    return int(rng[0]), dict(zip(TWIN_INTS, map(int, tw))), dict(zip(SEG_INTS, map(int, sg))), (BUILDERS[int(end[0])], int(end[1]), int(end[2]))


@functools.lru_cache(maxsize=None)
def routes():
    cs = C.route_cases()
    return cs, [parse_route(ln) for ln in run([route_line(*c[1:]) for c in cs])]


# ---------------------------------------------------------------- the builders
def test_the_route_of_every_case_is_the_restatements():
    cs, got = routes()
    seen = collections.Counter()
    for (name, S, K, T, clash, touches, h_mx), (rng_ok, tw, sg, (builder, built, unfit)) in zip(cs, got):
        what = (name, S, K, T, clash, touches, h_mx)
        assert rng_ok == C.range_ok(S), what
        want_tw = C.twin_route(S, K, T)
        assert {k: bool(tw[k]) for k in want_tw} == want_tw, (what, tw)
        assert tw["ne"] == C.rung(S.max_col, C.WAVE) and (tw["wpb"], tw["per_wave"], tw["lds_bytes"]) == C.twin_fill(tw["ne"], S.n_batches), (what, tw)
        want = C.route(S, K, T, clash, touches, h_mx)
        assert (builder, built, unfit) == (want["builder"], want["csc_built"], want["seg_unfit"]), (what, builder, built, unfit, want)
        assert bool(sg["consulted"]) == (want["builder"] != "twin"), what
        if sg["consulted"]:
            want_sg = C.seg_route(S, K, T)
            assert {k: int(sg[k]) for k in want_sg} == {k: int(v) for k, v in want_sg.items()}, (what, sg, want_sg)
        else:
            assert not any(sg[k] for k in SEG_INTS[1:15]), what
        assert sg["gives_up"] == (h_mx > C.SEG_CAP) and sg["ipt"] == C.rung(h_mx, C.BLOCK), what
        seen[builder] += 1
        seen["twin", tw["wanted"], tw["tried"], tw["clashed"]] += 1
        seen["ne", tw["ne"]] += 1
        seen["by_key", tw["by_key"]] += 1
        seen["build_first", tw["build_first"]] += 1
        if sg["tried"]:
            seen["fl", sg["fl"]] += 1
            seen["narrow", sg["narrow"]] += 1
            seen["ipt", sg["ipt"], sg["gives_up"]] += 1
            seen["S", sg["S"]] += 1
            seen["xcd", sg["xcd"]] += 1
        seen["seg", sg["consulted"], sg["tried"]] += 1
        seen["unfit", S.seg_unfit, unfit] += 1
    assert len(cs) > 1000
    assert all(seen[b] > 0 for b in BUILDERS), seen
    assert all(seen["twin", w, t, c] > 0 for w, t, c in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1))), seen
    assert all(seen["ne", ne] > 0 for ne in (4, 8, 16)) and seen["by_key", 0] > 0 and seen["by_key", 1] > 0 and seen["build_first", 1] > 0
    assert all(seen["fl", fl] > 0 for fl in (8, 9, 10, 11, 12)) and seen["narrow", 0] > 0 and seen["narrow", 1] > 0
    assert all(seen["ipt", i, 0] > 0 for i in (4, 8, 16)) and seen["ipt", 16, 1] > 0
    assert all(seen["S", s] > 0 for s in (1, 64, 256, 257, 1000)) and seen["xcd", 0] > 0 and seen["xcd", 1] > 0
    assert all(seen["seg", c, t] > 0 for c, t in ((0, 0), (1, 0), (1, 1)))
    assert all(seen["unfit", a, b] > 0 for a, b in ((0, 0), (0, 1), (1, 1)))


def test_every_answer_has_the_properties_a_launch_needs():
    cs, got = routes()
    n = 0
    for (name, S, K, T, clash, touches, h_mx), (rng_ok, tw, sg, (builder, built, unfit)) in zip(cs, got):
        what = (name, S, K, T, sg, tw)
        assert not (builder == "twin" and sg["tried"]), what  # never both: bucketing is not even consulted after the twin
        assert tw["tried"] <= tw["wanted"] and tw["build_first"] <= tw["wanted"], what
        if tw["tried"]:
            assert S.max_col <= C.CSC_MAX_COL and S.max_col <= tw["ne"] * C.WAVE and S.n_batches <= C.CSC_MAX_BATCHES, what
            assert tw["wpb"] * C.WAVE <= C.BLOCK and tw["per_wave"] >= 4 * tw["ne"] * C.WAVE + 2 * S.n_batches, what
        if sg["tried"]:
            n += 1
            assert 8 <= sg["fl"] <= 12 and sg["nbk"] == ((S.d - 1) >> sg["fl"]) + 1 <= C.SEG_MAX_BUCKETS and sg["cells"] == S.n_batches * sg["nbk"] <= 1 << 23, what
            assert sg["cpb"] * sg["S"] >= S.max_batch > (sg["cpb"] - 1) * sg["S"], what
            assert (1 << sg["pbits"]) >= S.max_batch and (1 << sg["qbits"]) >= S.max_row, what
            assert sg["pmask"] >= S.max_batch - 1 and sg["qmask"] >= S.max_row - 1, what  # positions and entries fit their fields
            if sg["narrow"]:  # narrow items fit in 32 bits: the feature's low bits end at bit fl + sh_fl
                assert sg["fl"] + sg["sh_fl"] <= 32 and sg["sh_fl"] == sg["sh_pos"] + sg["pbits"] and sg["sh_pos"] == sg["qbits"], what
            else:
                assert sg["fl"] + sg["sh_fl"] <= 64 and sg["sh_pos"] == sg["sh_fl"] - sg["sh_pos"] == C.SEG_POS_BITS, what
            if not sg["gives_up"]:
                assert h_mx <= sg["ipt"] * C.BLOCK and sg["ipt"] in (4, 8, 16), what
                # (k_seg_fill asks for dynamic LDS only: within the 64 KB a launch gets without asking for more)
                assert sg["fill_lds"] == C.seg_fill_lds(sg["fl"], sg["ipt"]) <= 64 * 1024, what
    assert n > 300


def test_the_twin_fill_lds_stays_within_48_kb():
    """k_csc_fill's comment says "at most 48 KB of LDS per workgroup", and twin_fill (plan_route.h) now chooses the wavefronts
    per workgroup by that bound: four, or two where four would ask for more.  Before, the choice was by the rung alone (two at 16
    entries per lane), and with 8 entries per lane (a longest column of 257 ... 512) and 512 batches four wavefronts asked for
    4 x 4 x (2048 + 2 x 512 + 2) = 49184 bytes, 32 bytes more than 48 x 1024; that one launch is two wavefronts and 24592 bytes
    now (tests/test_gpu_plan.py builds it: twin_batch_counts_ne8).  The largest requests left: 49152 bytes (8 per lane, 511
    batches), 40976 (16 per lane, 512 batches), 32800 (4 per lane, 512 batches)."""
    cs, got = routes()
    worst = collections.defaultdict(int)
    for (name, S, K, T, clash, touches, h_mx), (rng_ok, tw, sg, end) in zip(cs, got):
        if tw["tried"]:
            worst[tw["ne"], S.n_batches] = max(worst[tw["ne"], S.n_batches], tw["lds_bytes"])
    print(sorted(worst.items()))
    assert {ne for ne, _ in worst} == {4, 8, 16} and (8, 512) in worst and (8, 511) in worst
    over = {k: v for k, v in worst.items() if v > 48 * 1024}
    assert not over, over
    assert worst[8, 511] == 48 * 1024 and worst[8, 512] == 24592 and worst[16, 512] == 40976 and worst[4, 512] == 32800


# ---------------------------------------------------------------- bounds and keys
def test_batch_bounds_of_every_case_are_the_restatements():
    cs = C.bounds_cases()
    got = run(["B %d %d %d" % c for c in cs])
    for (ns, batch, fs), ln in zip(cs, got):
        eff, bp = C.batch_bounds(ns, batch, fs)
        nb = len(bp) - 1
        at = lambda i: bp[i] if 1 <= i <= nb else -1
        want = [eff, nb, max([b - a for a, b in zip(bp, bp[1:])], default=0), at(1), at(2), at(nb - 1), sum(bp)]
        assert [int(v) for v in ln.split()] == want, (ns, batch, fs, ln, want)
        assert (nb, want[2]) == C.batch_counts(ns, batch, fs)
        assert eff <= max(ns, 1) and nb <= C.batch_bound(ns, batch)  # what the kernels divide by is a position count; the bound holds
    assert {c[1] for c in cs} >= {1 << 32, (1 << 32) + 7, (1 << 63) - 1} and len(cs) > 150


def test_key_widths_of_every_case_are_the_restatements():
    cs = C.key_cases()
    got = run(["K %d %d %d %d %d" % c for c in cs])
    seen = collections.Counter()
    for (d, n_aug, ns, batch, fs), ln in zip(cs, got):
        t, s = ([int(v) for v in part.split()] for part in ln.split("|"))
        bound = C.batch_bound(ns, batch)
        nb, _ = C.batch_counts(ns, batch, fs)
        f, b, bits = C.key_bits(d, n_aug, bound)
        assert t == [bound, f, b, bits] and f + b == C.key_bit_sum(d, n_aug, ns, batch), (d, n_aug, ns, batch, fs, ln)
        fs_, bs_, _ = C.key_bits(d, n_aug, nb)
        assert s == [nb, bs_, fs_ + bs_, C.count_bits(bs_)], (d, n_aug, ns, batch, fs, ln)
        assert nb <= bound and s[2] <= t[1] + t[2] and s[2] <= (64 if bits == 64 else 32)  # the sort's bit range fits the key's type
        seen[bits, f + b] += 1
        seen["gap", t[2] - s[1]] += 1
    assert seen[32, 32] > 0 and seen[64, 33] > 0 and seen["gap", 0] > 0 and seen["gap", 1] > 0, seen
    assert [C.count_bits(b) for b in (1, 27, 28, 29, 31, 32)] == [4, 4, 4, 3, 1, 0]


# ---------------------------------------------------------------- the parent's lines; the knobs; the sources; the sanitizers
def clean_env():
    return {k: v for k, v in os.environ.items() if k not in C.KNOB_NAMES}


PARENT_RE = (r"draws (\d+) disagreements (\d+) \| twin (\d+) clashed (\d+) seg (\d+) gave_up (\d+) sort (\d+) \| key64 (\d+) errors (\d+) narrow (\d+) "
             r"wide (\d+) built_now (\d+) fill_corner (\d+)")


def test_the_header_against_the_lines_it_replaced():
    out = subprocess.run([exe(), "parent", "40000", "7"], capture_output=True, text=True, timeout=600, env=clean_env())
    assert out.returncode == 0 and "DISAGREE" not in out.stdout, out.stdout[-4000:]
    n = [int(v) for v in re.search(PARENT_RE, out.stdout).groups()]
    assert n[0] == 40000 and n[1] == 0
    assert min(n[2:-1]) > 100, out.stdout  # the draws reach what they compare: every builder, both fallbacks, both widths, the refusals
    assert n[-1] > 20, out.stdout  # ... and the one launch of k_csc_fill that is no longer the parent's (two wavefronts where four asked for 49184 bytes)


def test_the_knobs_are_read_from_the_environment():
    env = clean_env()
    for vals in ((None,) * 6, ("0", "0", "0", "8", "64", "0"), ("1", "1", "1", "13", "-2", "1"), ("", "x", "2", "-4", "6x", "")):
        e = dict(env, **{k: v for k, v in zip(C.KNOB_NAMES, vals) if v is not None})
        out = subprocess.run([exe(), "knobs"], capture_output=True, text=True, timeout=60, env=e)
        want = [UNSET if v is None else int(re.match(r"\s*[-+]?\d+", v).group()) if re.match(r"\s*[-+]?\d+", v) else 0 for v in vals]  # atoi
        assert out.returncode == 0 and [int(v) for v in out.stdout.split()] == want, (vals, out.stdout)
        assert tuple(C.knobs_of(e)) == tuple(None if v is None else w for v, w in zip(vals, want))


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_source_still_has_the_choices_restated():
    """the header is the one reader of the build's environment, plan.hip calls it, and only the sort builder is a template"""
    route, plan = src("plan_route.h"), src("plan.hip")
    assert "getenv" not in plan and route.count("getenv(") == 1 and all('"%s"' % k in route for k in C.KNOB_NAMES)
    for call in ("plan_knobs()", "twin_route(S, K, c.T)", "seg_route(S, K, c.T)", "twin_clashed(", "seg_gives_up(", "twin_ne(", "seg_ipt(", "plan_bounds(",
                 "plan_key(", "plan_count_bits(", "twin_fill("):
        assert call in plan, call
    assert "static_assert(kPlanWave == kWave && kPlanBlock == kBlock" in plan
    assert re.findall(r"template <class KeyT>\n(?:static |__global__ )(?:int|void) (\w+)", plan) == ["k_expand", "k_classify", "k_compact", "build_by_sort"]
    assert "plan_route.h" in src("Makefile").split("HDRS :=")[1].split("\n")[0]
    # the constants the restatement carries
    for text in ("kCscMaxCol = 1024;", "kCscMaxBatches = 512;", "kCscMaxCells = 268435456.0;", "kCscMinFill = 0.5;", "kCscFillLds = 48 * 1024;","kSegCap = 4096;", "kSegMaxBuckets = 4096;",
                 "kSegPosBits = 26, kSegFlShift = 52;", "kSegMaxCells = (int64_t)1 << 23;", "kSegMinTouches = 8192.0;", "kSegTarget = 2048.0;",
                 "kSegChunk = 256;", "kCntClassBits = 4,", "0.75 * kSegCap", "kPlanWave = 64;", "kPlanBlock = 256;"):
        assert text in route, text


def test_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined, on every 7th route case, all bounds and key cases and 4000 draws
    against the parent's lines: no report (a report ends it with a nonzero status), the same answers"""
    lines = [route_line(*c[1:]) for c in C.route_cases()[::7]] + ["B %d %d %d" % c for c in C.bounds_cases()] + ["K %d %d %d %d %d" % c for c in C.key_cases()]
    assert run(lines, sanitize=True) == run(lines)
    a = subprocess.run([exe(True), "parent", "4000", "3"], capture_output=True, text=True, timeout=600, env=clean_env())
    b = subprocess.run([exe(), "parent", "4000", "3"], capture_output=True, text=True, timeout=600, env=clean_env())
    assert a.returncode == 0 and a.stdout == b.stdout and "disagreements 0" in a.stdout, a.stdout[-2000:] + a.stderr[-4000:]
