"""-m gpu: newPSGD with newL1() / newL21() on the device (nimfm_amd/csrc/psgd_seq.hip) against the line-cited restatement of
optimizer/psgd.nim and the regularisers' lazy hooks (tests/psgd_lazy_restatement.py; L1's cache reset under "consistent", the
departure DESIGN.md section 22 states).  The cases are tests/psgd_lazy_cases.py's; tests/test_psgd_lazy_restatement.py holds
what makes these comparisons meaningful (every threshold taken is at least 1e-6 away, relatively, from the magnitude it
cuts: the zero pattern is compared with no entry exempt).

Bounds: P, w, the intercept and the per-epoch loss sums at rtol 1e-9 / atol 1e-12, the bound of __graft_entry__.smoke for the
reference's exact order.  In the two reset cases P collapses to 1e-10 and below, so P's atol there is 1e-12 * max|P| of the
restatement."""
import ctypes as C

import numpy as np
import pytest

import nimfm_amd as nf
import psgd_lazy_cases as CS
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
REG = {"l1": nf.newL1, "l21": nf.newL21}
HOST_NAMES = {"loss_param": "lossParam"}


def _dataset(case):
    X = case.X
    return nf.newCSRDataset(X.data, X.indices, X.indptr, X.n, X.d)


def _model(case, warmStart=True):
    m = case.model
    fm = nf.newFactorizationMachine(m["task"], degree=m["degree"], nComponents=case.k, fitLower=m["fit_lower"],
                                    fitIntercept=m["fit_intercept"], fitLinear=m["fit_linear"], warmStart=warmStart)
    fm.set_params(case.P0.copy(), case.w0.copy(), case.b0)
    return fm


def _solver(case, reg, **over):
    kw = {HOST_NAMES.get(k_, k_): v for k_, v in case.solver.items()}
    kw.update(verbose=0, reg=REG[reg](), shuffle=False)
    kw.update(over)
    return nf.newPSGD(**kw)


def _fit(case, reg, **over):
    X, fm, opt = _dataset(case), _model(case), _solver(case, reg, **over)
    opt.fit(X, case.y, fm, perms=case.perms)
    return X, fm, opt


def _assert_equal(fm, loss_sums, ref, what, p_atol=ATOL):
    print("%s: max|dP| %.3e (max|P| %.3e)  max|dw| %.3e  |db| %.3e  zeros %d/%d" % (
        what, np.abs(fm.P - ref.P).max(), np.abs(ref.P).max(), np.abs(fm.w - ref.w).max(), abs(fm.intercept - ref.intercept),
        int((fm.P == 0).sum()), fm.P.size))
    assert np.isfinite(ref.P).all(), what
    np.testing.assert_allclose(fm.P, ref.P, rtol=RTOL, atol=p_atol, err_msg=what)
    np.testing.assert_allclose(fm.w, ref.w, rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_allclose(fm.intercept, ref.intercept, rtol=RTOL, atol=ATOL, err_msg=what)
    assert np.array_equal(fm.P == 0.0, ref.P == 0.0), "%s: the sets of exact zeros differ" % what
    if loss_sums is not None:
        np.testing.assert_allclose(loss_sums, ref.losses, rtol=RTOL, atol=ATOL, err_msg=what)


def _check(case, reg, p_atol=None):
    ref = case.reference(reg)
    _, fm, opt = _fit(case, reg)
    _assert_equal(fm, opt.lossSums, ref, "%s/%s" % (case.name, reg), ATOL if p_atol is None else p_atol * np.abs(ref.P).max())
    assert opt.it == ref.it
    return fm, opt, ref


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("grid", CS.GRID, ids=lambda g: "deg%d-%s-lin%d-int%d" % g)
def test_grid(grid, reg):
    """the reference's grid (test_psgd_l1.nim:99-135): degrees 2 to 4, fitLower x fitLinear x fitIntercept, 5 epochs"""
    case = CS.grid_case(*grid)
    fm, _, _ = _check(case, reg)
    if not case.model["fit_linear"]:
        assert not fm.w.any()  # test_psgd_l1.nim:18-38
    if not case.model["fit_intercept"]:
        assert fm.intercept == 0.0  # :41-60


@pytest.mark.parametrize("name,reg", list(CS.SPARSE), ids=lambda v: str(v))
def test_sparse(name, reg):
    fm, _, _ = _check(CS.sparse_case(name, reg), reg)
    assert 0.2 <= (fm.P == 0).mean() <= 0.8


@pytest.mark.parametrize("reg", CS.REGS)
def test_cache_reset(reg):
    """the regulariser's scaling passes 1e-8: the persistent kernel stops, the dense pass runs, the walk goes on"""
    fm, _, ref = _check(CS.cache_reset_case(), reg, p_atol=1e-12)
    assert ref.record.cache_resets >= 1 and fm.P.any()


@pytest.mark.parametrize("reg", CS.REGS)
def test_w_reset(reg):
    _, _, ref = _check(CS.w_reset_case(), reg, p_atol=1e-12)
    assert ref.record.w_resets >= 1


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("loss", CS.LOSSES)
def test_losses(loss, reg):
    _check(CS.loss_case(loss), reg)


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("name", list(CS.SCHEDULES))
def test_schedules(name, reg):
    _check(CS.schedule_case(name), reg)


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("k", CS.WIDTHS)
def test_widths(k, reg):
    """below one wavefront, exactly one, one factor more (L21's row norm goes on across the wavefronts in order), two"""
    _check(CS.width_case(k), reg)


@pytest.mark.parametrize("reg", CS.REGS)
@pytest.mark.parametrize("kind", CS.ROW_KINDS)
def test_row_lengths(kind, reg):
    _check(CS.row_case(kind), reg)


@pytest.mark.parametrize("reg", CS.REGS)
def test_long_rows(reg):
    """200 entries per row at k = 64: the per-sample table is in global memory"""
    _check(CS.long_row_case(), reg)


# ---- the C ABI's calls by hand: sub-ranges, caches, finalize ----
class _Manual:
    def __init__(self, case, reg, **over):
        self.case, self.X, self.fm = case, _dataset(case), _model(case)
        self.opt = _solver(case, reg, **over)
        self.fm.init(self.X)
        self.X.set_targets(np.asarray(case.y, dtype=np.float64))
        self.opt._handle(self.fm, self.X.ctx, "sequential")
        self.L = capi.lib()
        capi.check(self.L.nfm_opt_set_it(self.opt._h, 1))
        capi.check(self.L.nfm_psgd_begin_fit(self.opt._h, self.X.h))
        self.loss = 0.0

    def run(self, perm, begin, end):
        ls, vs = self.opt._epoch(self.X, perm, begin, end)
        assert vs == 0.0
        self.loss += ls
        return ls

    def finalize(self):
        capi.check(self.L.nfm_psgd_finalize(self.opt._h))
        self.fm._pull()
        return self.fm


@pytest.mark.parametrize("reg", CS.REGS)
def test_caches_carry_over_sub_range_calls(reg):
    """[0, 37) and [37, 80) as two calls without finalize: the snapshot arrays and the three scalars one call leaves are what
    the next one starts from -- the parameters are BITWISE those of the single call [0, 80), and equal the restatement's"""
    case = CS.grid_case(3, "augment", True, True)
    perm = np.ascontiguousarray(case.perms[0])
    one, two = _Manual(case, reg), _Manual(case, reg)
    one.run(perm, 0, 80)
    two.run(perm, 0, 37)
    two.run(perm, 37, 80)
    a, b = one.finalize(), two.finalize()
    assert np.array_equal(a.P, b.P) and np.array_equal(a.w, b.w) and a.intercept == b.intercept
    ref = case.restate(reg, maxIter=1, perms=case.perms[:1])
    _assert_equal(b, [two.loss], ref, "two calls/%s" % reg)
    _assert_equal(a, [one.loss], ref, "one call/%s" % reg)


@pytest.mark.parametrize("reg", CS.REGS)
def test_sub_ranges_with_finalize_equal_ncalls(reg):
    """psgd.nim:179-182 with nCalls = 37: finalize runs after the 37th and the 74th sample (it mod nCalls == 0), so the epoch is
    [0, 37), finalize, [37, 74), finalize, [74, 80) -- through the C ABI by hand, and through fit with a callback.  L21's
    lazyUpdateFinal leaves its caches as they are (l21.nim:72-78): kept, the restatement has the same lines"""
    case = CS.grid_case(3, "augment", True, True)
    perm = np.ascontiguousarray(case.perms[0])
    seen = []
    ref = case.restate(reg, maxIter=1, perms=case.perms[:1], nCalls=37, callback=lambda it, P, w, b: seen.append((it, P, w, b)))
    assert [s[0] for s in seen] == [37, 74]
    man = _Manual(case, reg)
    man.run(perm, 0, 37)
    mid = man.finalize()
    np.testing.assert_allclose(mid.P, seen[0][1], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mid.w, seen[0][2], rtol=RTOL, atol=ATOL)
    man.run(perm, 37, 74)
    man.finalize()
    man.run(perm, 74, 80)
    _assert_equal(man.finalize(), [man.loss], ref, "by hand/%s" % reg)
    got = []
    X, fm, opt = _dataset(case), _model(case), _solver(case, reg, maxIter=1, nCalls=37)
    opt.fit(X, case.y, fm, perms=case.perms[:1], callback=lambda o, m: got.append((o.it, m.P.copy(), m.w.copy(), m.intercept)))
    assert [g[0] for g in got] == [37, 74]
    for g, s in zip(got, seen):
        np.testing.assert_allclose(g[1], s[1], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g[2], s[2], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g[3], s[3], rtol=RTOL, atol=ATOL)
    _assert_equal(fm, opt.lossSums, ref, "callback fit/%s" % reg)
    assert np.array_equal(fm.P, man.fm.P) and np.array_equal(fm.w, man.fm.w)


@pytest.mark.parametrize("reg", CS.REGS)
def test_warm_start(reg):
    """test_psgd_l1.nim:63-96: ten fits of one epoch equal one fit of ten epochs (shuffle = false), atol 1e-8 -- `it` persists
    between fits, the caches are re-initialised by every fit"""
    case = CS.grid_case(3, "explicit", True, True)
    X = _dataset(case)
    warm, opt = _model(case, warmStart=True), _solver(case, reg, maxIter=1)
    for _ in range(10):
        opt.fit(X, case.y, warm)
    assert opt.it == 801
    once = _model(case, warmStart=True)
    _solver(case, reg, maxIter=10).fit(X, case.y, once)
    print("warm start/%s: max|dP| %.3e" % (reg, np.abs(warm.P - once.P).max()))
    assert abs(warm.intercept - once.intercept) < 1e-8
    np.testing.assert_allclose(warm.w, once.w, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(warm.P, once.P, rtol=1e-6, atol=1e-8)
    cold = _model(case, warmStart=False)  # not warmStart: it starts again at 1 (psgd.nim:106-107)
    opt.fit(X, case.y, cold)
    assert opt.it == 81


@pytest.mark.parametrize("reg", CS.REGS)
def test_decision_function_and_determinism(reg):
    case = CS.sparse_case("sparse-deg3", reg)
    X, fm, _ = _fit(case, reg)
    _, fm2, _ = _fit(case, reg)
    assert np.array_equal(fm.P, fm2.P) and np.array_equal(fm.w, fm2.w) and fm.intercept == fm2.intercept  # bitwise
    Xd = case.X.dense()
    want = fm.intercept + Xd @ fm.w
    deg = case.model["degree"]
    for order in range(fm.P.shape[0]):  # the ANOVA kernel by its recursion (kernels.nim:46-64)
        for s in range(fm.P.shape[1]):
            A = np.zeros((X.nSamples, deg - order + 1))
            A[:, 0] = 1.0
            for j in range(Xd.shape[1]):
                for t in range(deg - order, 0, -1):
                    A[:, t] += A[:, t - 1] * fm.P[order, s, j] * Xd[:, j]
            want = want + A[:, deg - order]
    np.testing.assert_allclose(fm.decisionFunction(X), want, rtol=1e-9, atol=1e-12)


def test_refusals():
    """everything the scope leaves out, through the C ABI (NFM_ERR_UNSUPPORTED) and through newPSGD (ValueError)"""
    case = CS.grid_case(2, "explicit", True, True)
    X, L = _dataset(case), capi.lib()

    def create(fm, reg, ds=None):
        fm.init(ds or X)
        cfg = capi.MBPSGDCfg(0.01, 1e-6, 1e-3, 1e-4, 1e-4, 1.0, 1.0, 0, 1, capi.REG[reg], 0, 1)
        h = C.c_void_p()
        rc = L.nfm_psgd_create(fm._push((ds or X).ctx), C.byref(cfg), C.byref(h))
        return rc, h, L.nfm_last_error().decode()

    for reg, ctor in (("squaredl12", nf.newSquaredL12), ("squaredl21", nf.newSquaredL21)):
        rc, _, msg = create(_model(case), reg)
        assert rc == capi.ERR_UNSUPPORTED and "newMBPSGD" in msg
        with pytest.raises(ValueError, match="newMBPSGD"):
            nf.newPSGD(verbose=0, reg=ctor()).fit(X, case.y, _model(case))
    with pytest.raises(ValueError, match="newMBPSGD"):  # newPSGD()'s default regulariser is newSquaredL12() (psgd.nim:25)
        nf.newPSGD(verbose=0).fit(X, case.y, _model(case))
    for reg, ctor in (("omegati", nf.newOmegaTI), ("omegacs", nf.newOmegaCS)):
        rc, _, msg = create(_model(case), reg)
        assert rc == capi.ERR_UNSUPPORTED and "no SGD hooks" in msg
        with pytest.raises(ValueError, match="no SGD hooks"):
            nf.newPSGD(verbose=0, reg=ctor()).fit(X, case.y, _model(case))
    # a field-aware model
    fields = (case.X.indices % 2).astype(np.int64)
    Xf = nf.newCSRFieldDataset(case.X.data, case.X.indices, case.X.indptr, fields, case.X.n, case.X.d, 2)
    ffm = nf.newFieldAwareFactorizationMachine("regression", nComponents=4)
    rc, _, msg = create(ffm, "l1", Xf)
    assert rc == capi.ERR_UNSUPPORTED and "FactorizationMachine" in msg
    with pytest.raises(ValueError, match="newSGD"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(Xf, case.y, ffm)
    # nComponents > 128
    wide = nf.newFactorizationMachine("regression", degree=2, nComponents=129)
    rc, _, msg = create(wide, "l1")
    assert rc == capi.ERR_UNSUPPORTED and "n_components <= 128" in msg
    with pytest.raises(ValueError, match="nComponents <= 128"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(X, case.y, nf.newFactorizationMachine("regression", nComponents=129))
    # a streamed dataset, several devices: the host's refusals (the C ABI has no such arguments)
    with pytest.raises(ValueError, match="StreamCSRDataset"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(object.__new__(nf.StreamCSRDataset), case.y, _model(case))
    with pytest.raises(ValueError, match="devices"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(X, case.y, _model(case), devices=[0, 0])
    # a repeated id in a row, as newSGD refuses it
    rep = nf.newCSRDataset(np.array([1.0, 2.0, 3.0]), np.array([0, 0, 1]), np.array([0, 2, 3]), 2, case.X.d)
    keep = _model(case)  # (the optimizer refers to its model: it must outlive the calls below)
    rc, h, _ = create(keep, "l1")
    assert rc == 0
    rep.set_targets(np.zeros(2))
    assert L.nfm_psgd_begin_fit(h, rep.h) == capi.ERR_UNSUPPORTED and b"repeated column ids" in L.nfm_last_error()
    # an epoch call without begin_fit
    ls, vs = C.c_double(), C.c_double()
    X.set_targets(np.asarray(case.y, dtype=np.float64))
    assert L.nfm_opt_epoch(h, X.h, None, 0, 80, C.byref(ls), C.byref(vs)) == capi.ERR_INVALID
    L.nfm_opt_destroy(h)
    with pytest.raises(nf.NfmError, match="repeated column ids"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(rep, np.zeros(2), _model(case))


def test_cli(tmp_path):
    from test_gpu_pcd import _cli, _files
    train = _files(tmp_path)
    dump = str(tmp_path / "fm.txt")
    args = ["train", "--task", "r", "--train", train, "--solver", "psgd", "--reg", "l1", "--gamma", "1e-3", "--eta0", "0.05",
            "--scheduling", "optimal", "--power", "1.0", "--maxIter", "3", "--nComponents", "3", "--verbose", "0", "--shuffle", "false",
            "--dump", dump]
    r = _cli(args)
    assert r.returncode == 0, r.stderr
    got = nf.load(dump, False)
    X, y = nf.loadSVMLightFile(train, -1)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3, randomState=1, scale=0.1)
    nf.newPSGD(maxIter=3, eta0=0.05, alpha0=1e-7, alpha=1e-5, beta=1e-3, gamma=1e-3, reg=nf.newL1(), verbose=0, tol=1e-5,
               shuffle=False, lossParam=0.1).fit(X, y, fm)
    ref = str(tmp_path / "ref.txt")
    fm.dump(ref)
    want = nf.load(ref, False)  # through the same text format: the dump's digits are what is compared
    assert np.array_equal(got.P, want.P) and np.array_equal(got.w, want.w) and got.intercept == want.intercept
    assert np.isfinite(got.P).all() and got.P.any()
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "psgd", "--reg", "squaredl12", "--nComponents", "3"])
    assert r.returncode != 0 and "newMBPSGD" in r.stderr
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "cd"])  # still refused, with its own message
    assert r.returncode != 0 and "not supported" in r.stderr
