"""newHazan, newGreedyCD and the convex model's decisionFunction on the device beyond one trip of fin_sum and one captured
chunk: the inputs of tests/cfm_grid_cases.py against the restatements (tests/hazan_restatement.py, tests/gcd_restatement.py).

The method and the tolerances are tests/test_gpu_hazan.py's and tests/test_gpu_gcd.py's, imported from there: the plain
restatement first with the CG counts within one, then the restatement forced to the device's counts; P and w at rtol 1e-6 /
atol 1e-9, lams at 1e-7, the intercept at 1e-5, loss, step and the objectives at 1e-8 relative.
tests/test_cfm_grid_cases.py asserts on the CPU what each input reaches and guards its conditioning."""
import functools

import numpy as np
import pytest

import cfm_direct_child
import cfm_grid_cases as G
import gcd_restatement as gr
import hazan_cases as hc
import hazan_restatement as hr
import test_cfm_grid_cases as Tc
import test_gpu_gcd as TG
import test_gpu_hazan as TH

pytestmark = pytest.mark.gpu
kHazanChunk = Tc.kHazanChunk  # read out of cfm.h


@pytest.fixture(scope="module")
def nf():
    import __graft_entry__ as g
    g.build()
    import nimfm_amd
    return nimfm_amd


def _ids(runs):
    return ["%s-%s" % (n, "".join("FT"[f] for f in fl)) for n, fl in runs]


def _start_feed(count):
    starts, k = hc.numpy_starts(G.START_SEED), iter(range(count))
    return lambda d: starts(next(k), d)


def hazan_device_fit(nf, name, flags, cfm=None, opt=None, **over):
    X, y, kw, _ = G.hazan_case(name, flags, **over)
    return TH._device_fit(nf, X, y, kw, powerInit=_start_feed(kw["maxIter"]), cfm=cfm, opt=opt)


def gcd_device_fit(nf, name, cfm=None):
    X, y, kw = G.gcd_case(name)
    return TG._device_fit(nf, X, y, kw, cfm=cfm, powerInit=_start_feed(kw["maxIter"] * kw["maxIterInner"]), seed=None)


def _hazan_parity(nf, name, flags, maxIterPower=None):
    """test_wide_case's method -> (model, solver, the restatement forced to the device's counts)"""
    over = {} if maxIterPower is None else dict(maxIterPower=maxIterPower)
    X, y, kw, starts = G.hazan_case(name, flags, **over)
    cfm, opt = hazan_device_fit(nf, name, flags, **over)
    plain = G.hazan_plain(name, flags, maxIterPower)
    assert len(opt.history) == len(plain.history)
    for got, want in zip(opt.history, plain.history):
        print("%s: cg iterations device %d, restatement %d; power iterations %d" % (name, got["cgIters"], want["cgIters"], got["powerIters"]))
        assert abs(got["cgIters"] - want["cgIters"]) <= 1, (got, want)
    forced = [(r["powerIters"], r["cgIters"]) for r in opt.history]
    same = forced == [(r["powerIters"], r["cgIters"]) for r in plain.history]
    ref = plain if same else hr.hazan_fit(X, y, starts, forced=forced, **kw)  # forcing the plain run's own counts reproduces it
    print("%s: max |dP| %.3e  |dw| %.3e  |dlams| %.3e  |db| %.3e  loss %.3e" % (
        name, np.abs(cfm.P - ref.P).max(), np.abs(cfm.w - ref.w).max(), np.abs(cfm.lams - ref.lams).max(), abs(cfm.intercept - ref.intercept),
        max(abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(opt.history, ref.history))))
    TH._check_model(cfm, ref)
    TH._check_records(opt.history, ref.history)
    if not kw["fitLinear"]:
        assert not cfm.w.any()
        if not kw["fitIntercept"]:
            assert cfm.intercept == 0.0
    return cfm, opt, ref


@pytest.mark.parametrize("name,flags", G.HAZAN_RUNS, ids=_ids(G.HAZAN_RUNS))
def test_hazan(nf, name, flags):
    """tall: 1026 workgroups of rows; long: 1026 element-wise workgroups over n; broad: mass behind partial 1024 of the passes
    over d and d + 1; the edge shapes: the last workgroup of every pass one below, on and one above 32 and 256"""
    cfm, opt, ref = _hazan_parity(nf, name, flags)
    assert len(opt.history) == G.HAZAN[name]["maxIter"] and np.isfinite(cfm.P).all()
    if flags[2]:
        assert max(r["cgIters"] for r in opt.history) > 1
    if name == "broad":
        far = slice(G.BROAD_BANDS[2][0], G.BROAD_BANDS[2][1])
        assert np.abs(cfm.P[:, far]).max() >= 0.01 * np.abs(cfm.P).max()


def test_cg_long(nf):
    """a second captured chunk of CG with the stop inside it"""
    cfm, opt, ref = _hazan_parity(nf, *G.CG_LONG_RUN)
    assert len(opt.history) == 1 and opt.history[0]["cgIters"] > kHazanChunk


def test_cg_cap(nf):
    """10 000 x 30 000: the CG ends on its cap of kCgMaxIter iterations, inside a chunk.  A CG that long is chaotic under
    rounding, so nothing is held to the restatement but the count; everything is finite and two runs are bit-equal.  The CPU
    file holds the restatement 10x above the CG's tolerance at the cap under both summations."""
    runs = [hazan_device_fit(nf, *G.CG_CAP_RUN) for _ in range(2)]
    for cfm, opt in runs:
        r = opt.history[0]
        assert len(opt.history) == 1 and r["cgIters"] == Tc.kCgMaxIter == G.hazan_plain(*G.CG_CAP_RUN).history[0]["cgIters"]
        assert np.isfinite(cfm.P).all() and np.isfinite(cfm.w).all() and np.isfinite(cfm.intercept) and np.isfinite(r["loss"])
    assert _bits(*runs[0]) == _bits(*runs[1])


@pytest.mark.parametrize("maxIterPower", G.POWER_EDGES)
def test_power_chunk_edges(nf, maxIterPower):
    """tolPower = 0 on the reference grid: the cap ends the power method one below, on and one above a chunk's end"""
    cfm, opt, ref = _hazan_parity(nf, "grid", G.POWER_EDGE_FLAGS, maxIterPower)
    assert [r["powerIters"] for r in opt.history] == [maxIterPower] * 2


@functools.lru_cache(maxsize=None)
def _gcd_reference(name, forced_key):
    X, y, kw = G.gcd_case(name)
    forced = dict(power=list(forced_key[0]), inner=list(forced_key[1]), outer=forced_key[2])
    return gr.gcd_fit(X, y, hc.numpy_starts(G.START_SEED), summation="tree", forced=forced, **kw)


def _gcd_parity(nf, name):
    """tests/test_gpu_gcd.py's _run_case on the inputs of this file"""
    cfm, opt = gcd_device_fit(nf, name)
    ref = _gcd_reference(name, TG._key(gr.counts_of(opt.history)))
    TG._check_model(name, cfm, ref)
    TG._check_records(opt.history, ref.history)
    return cfm, opt, ref, G.gcd_case(name)[2]


@pytest.mark.parametrize("name", G.GCD_CASES)
def test_gcd(nf, name):
    cfm, opt, ref, kw = _gcd_parity(nf, name)
    assert any(r["refit"] for r in TG._inner(opt.history)) and cfm.nComponents == kw["maxComponents"]
    assert gr.counts_of(opt.history)["power"] == [kw["maxIterPower"]] * kw["maxComponents"]


def test_gcd_power_chunk_edge(nf):
    cfm, opt, ref, kw = _gcd_parity(nf, G.GCD_GRID_CASE)
    counts = gr.counts_of(opt.history)["power"]
    assert counts and set(counts) == {G.GCD_POWER_EDGE}


def test_launch_by_launch_equals_the_graph(nf, tmp_path):
    """NFM_HAZAN_GRAPH=0 in a fresh child process: cg_long and a GreedyCD grid case, bit for bit the captured chunks' results"""
    cfm_direct_child.compare(tmp_path, kHazanChunk)


def _bits(cfm, opt):
    return (cfm.P.tobytes(), cfm.lams.tobytes(), cfm.w.tobytes(), float(cfm.intercept), repr(opt.history))


def test_state_reuse_hazan(nf):
    """The device solver belongs to one device model, and that to one width.  So one newHazan and one model fit tall, then the
    257 rows of `reuse` (the same width: the same device solver, vec, part and scal reused, the captured chunks dropped), then
    tall again; each result is a fresh solver's on a fresh model.  Then the same solver fits the reference grid into a fresh
    model (another width: a new device solver behind the same host object)."""
    flags = (True, True, True, True)
    kw = G.hazan_case("tall", flags)[2]
    opt = nf.newHazan(maxIter=kw["maxIter"], eta=kw["eta"], verbose=0, tol=kw["tol"], maxIterPower=kw["maxIterPower"], tolPower=0.0, optimal=True)
    cfm = nf.newConvexFactorizationMachine("regression", maxComponents=kw["maxComponents"])
    hazan_device_fit(nf, "tall", flags, cfm=cfm, opt=opt)
    big = _bits(cfm, opt)
    handle = opt._h.value
    hazan_device_fit(nf, "reuse", flags, cfm=cfm, opt=opt)
    assert opt._h.value == handle and cfm.P.shape == (3, G.SHAPES["reuse"][1])  # the same device solver
    assert _bits(cfm, opt) == _bits(*hazan_device_fit(nf, "reuse", flags))
    hazan_device_fit(nf, "tall", flags, cfm=cfm, opt=opt)
    assert opt._h.value == handle and _bits(cfm, opt) == big == _bits(*hazan_device_fit(nf, "tall", flags))
    over = dict(maxIterPower=kw["maxIterPower"], maxIter=kw["maxIter"], eta=kw["eta"], maxComponents=kw["maxComponents"])
    small, _ = hazan_device_fit(nf, "grid", flags, opt=opt, **over)
    assert small is not cfm and _bits(small, opt) == _bits(*hazan_device_fit(nf, "grid", flags, **over))


def test_state_reuse_gcd(nf):
    """the same for GreedyCD: tall, then `reuse` on the same solver and model, then its reference grid into a fresh model"""
    kw = G.gcd_case("tall:11")[2]
    fresh_opt = lambda: nf.newGreedyCD(maxIter=2, alpha0=kw["alpha0"], alpha=kw["alpha"], beta=kw["beta"], maxIterInner=kw["maxIterInner"],
                                       nRefitting=kw["nRefitting"], verbose=0, tol=kw["tol"], maxIterPower=G.GCD_POWER_EDGE,
                                       tolPower=kw["tolPower"])
    opt = fresh_opt()
    model = lambda k: nf.newConvexFactorizationMachine("regression", maxComponents=k)

    def fit(o, m, name):
        X, y = G.data(name) if name != "grid" else hc.grid_data(True, True)
        o.fit(TG._dataset(nf, X), y, m, powerInit=_start_feed(64))
        return _bits(m, o)

    cfm = model(3)
    big = fit(opt, cfm, "tall")
    handle = opt._h.value
    assert fit(opt, cfm, "reuse") == fit(fresh_opt(), model(3), "reuse") and opt._h.value == handle
    assert fit(opt, cfm, "tall") == big and opt._h.value == handle
    assert fit(opt, model(6), "grid") == fit(fresh_opt(), model(6), "grid")


def test_two_runs_of_broad_are_bitwise_equal(nf):
    flags = (True, True, True, True)
    a, b = (_bits(*hazan_device_fit(nf, "broad", flags)) for _ in range(2))
    assert a == b
    a, b = (_bits(*gcd_device_fit(nf, "broad:11")) for _ in range(2))
    assert a == b


@pytest.mark.parametrize("rows", ["tall", "predict33"])
@pytest.mark.parametrize("ignoreDiag", [True, False])
def test_decision_function(nf, rows, ignoreDiag):
    """k_cfm_predict on every row length of the cycle, on the training matrix's shape and on 33 other rows, with 0, 1 and 3
    components: the row sums are in the reference's order and nothing is contracted, so the values are the restatement's"""
    X, _ = G.data(rows)
    ds = TH._dataset(nf, X)
    for P, lams, w, b in G.predict_models(X.d, G.SHAPES["tall"][2]):
        cfm = nf.newConvexFactorizationMachine("regression", maxComponents=4, ignoreDiag=ignoreDiag)
        cfm.set_params(P, lams, w, b)
        got = cfm.decisionFunction(ds)
        want = hr.decision_function(X, P, lams, w, b, ignoreDiag)
        err = np.abs(got - want)
        print("%s, %d components, ignoreDiag %s: %d of %d values differ, max relative distance %.3e" % (
            rows, len(lams), ignoreDiag, int((got != want).sum()), X.n, float((err / np.abs(want)).max())))
        assert got.shape == (X.n,) and (err <= 1e-12 * np.abs(want)).all()
