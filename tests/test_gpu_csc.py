"""-m gpu: column-major datasets on the device (nimfm_amd/csrc/dataset_csc.hip) against the
plain-Python restatement of the reference's procs (tests/csc_restatement.py), bit for bit: np.array_equal on every array of
every result.  The cases are tests/csc_cases.py's; tests/test_csc_restatement.py holds the restatement to dense numpy.

Nothing here has a tolerance: the ops are copies, integer work and in-order folds, and what a consumer of rows computes on a
CSCDataset is what it computes on toCSRDataset of it -- the same kernels on the same bytes."""
import ctypes as C

import numpy as np
import pytest

import csc_cases as K
import csc_restatement as R
import dataset_ops_cases as KK
import dataset_ops_restatement as RR
import nimfm_amd as nf
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
NORMS = ("l1", "l2", "linfty")
I64 = np.int64


def up(X):
    ds = nf.newCSRDataset(np.array(X.data), np.array(X.indices, dtype=I64), np.array(X.indptr, dtype=I64), X.n, X.d)
    if X.y is not None:
        ds.set_targets(np.array(X.y))
    return ds


def up_csc(Cm):
    ds = nf.newCSCDataset(np.array(Cm.data), np.array(Cm.indices, dtype=I64), np.array(Cm.indptr, dtype=I64), Cm.n, Cm.d)
    if Cm.y is not None:
        ds.set_targets(np.array(Cm.y))
    return ds


def _targets(ds, ref, what):
    if ref.y is None:
        with pytest.raises(ValueError, match="no targets"):
            ds.targets()
    else:
        assert np.array_equal(ds.targets(), np.array(ref.y)), what


def same_csc(ds, ref, what=""):
    assert isinstance(ds, nf.CSCDataset), what
    indptr, indices, data = ds.to_host()
    assert ds.shape == [ref.n, ref.d] and ds.nFeatures == ref.d and ds.nnz == ref.nnz, what
    assert np.array_equal(indptr, np.array(ref.indptr, dtype=I64)), what
    assert np.array_equal(indices, np.array(ref.indices, dtype=I64)), what
    assert np.array_equal(data, np.array(ref.data, dtype=np.float64)), what
    _targets(ds, ref, what)


def same_csr(ds, ref, what=""):
    assert type(ds) is nf.CSRDataset, what
    indptr, indices, data, fields = ds.to_host()
    assert ds.shape == [ref.n, ref.d] and ds.nnz == ref.nnz and fields is None, what
    assert np.array_equal(indptr, np.array(ref.indptr, dtype=I64)), what
    assert np.array_equal(indices, np.array(ref.indices, dtype=I64)), what
    assert np.array_equal(data, np.array(ref.data, dtype=np.float64)), what
    _targets(ds, ref, what)


def _all_cases():
    out = dict(K.small_cases())
    out["long"] = K.long_case()
    out["dense"] = K.dense_case()
    return out


ALL = _all_cases()


@pytest.mark.parametrize("name", sorted(ALL))
def test_transpositions(name):
    """the literal, n = 1, d = 1, nnz = 0, empty rows and columns, unsorted rows, a row repeating an id, d > n, n > d, columns of
    9 / 70 / 1100 entries (lane group, wavefront), segments that average 64 entries or more"""
    X = ALL[name]
    ds = up(X)
    dc = nf.toCSCDataset(ds)
    ref = R.to_csc(X)
    same_csc(dc, ref, name)
    same_csr(nf.toCSRDataset(dc), R.to_csr(ref), name)
    same_csr(ds, X, "the input is unchanged")
    # an uploaded CSCDataset is the same object as a converted one
    same_csc(up_csc(ref), ref, name)
    same_csr(nf.toCSRDataset(up_csc(ref)), R.to_csr(ref), name)
    # two transpositions of the same input are byte-equal
    again = nf.toCSCDataset(ds)
    for a, b in zip(dc.to_host(), again.to_host()):
        assert a.tobytes() == b.tobytes()
    # conversions to the layout a dataset already has are copies
    same_csc(nf.toCSCDataset(dc), ref, name)
    same_csr(nf.toCSRDataset(ds), X, name)


def test_repeat_in_a_column_keeps_column_storage_order():
    indptr, indices, data, n, d = K.repeat_in_column_csc()
    ref = R.Csc(indptr, indices, data, n, d, y=[1.0, 2.0, 3.0, 4.0])
    dc = up_csc(ref)
    same_csc(dc, ref)
    same_csr(nf.toCSRDataset(dc), R.to_csr(ref))


def _hip_runtime():
    """the HIP runtime the library itself is linked to (the one already loaded into this process)"""
    capi.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "libnimfm_hip.so loaded no libamdhip64"
    return C.CDLL(paths[0])


def test_from_device():
    """column arrays that already live in HBM: the dataset copies them, so they may be freed at once"""
    hip = _hip_runtime()
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    ref = R.to_csc(ALL["unsorted_rows"])
    host = [np.array(ref.indptr, dtype=I64), np.array(ref.indices, dtype=np.int32), np.array(ref.data), np.array(ref.y)]
    dev = []
    for a in host:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        dev.append(p)
    dc = nf.CSCDataset.from_device(nf.default_context(), ref.n, ref.d, ref.nnz, *[p.value for p in dev])
    for p in dev:
        assert hip.hipFree(p) == 0
    same_csc(dc, ref)
    same_csr(nf.toCSRDataset(dc), R.to_csr(ref))


@pytest.mark.parametrize("name", ["literal", "unsorted_rows", "long", "dense", "empty_rows_and_columns", "repeat_in_row"])
def test_slices(name):
    """a slice of everything, slices that empty some columns, one row; the ids are rebased and the targets sliced"""
    X = ALL[name]
    ref = R.to_csc(X)
    dc = up_csc(ref)
    grid = K.literal_slices() if name == "literal" else [(0, X.n), (X.n // 3, X.n // 3 + 1), (X.n // 4, 3 * X.n // 4 + 1), (X.n - 1, X.n)]
    for a, b in grid:
        got = dc[a:b]
        want = R.slice_rows(ref, a, b)
        same_csc(got, want, "%s[%d:%d]" % (name, a, b))
        same_csr(nf.toCSRDataset(got), R.to_csr(want), "%s[%d:%d]" % (name, a, b))
    same_csc(dc[range(0, 1)], R.slice_rows(ref, 0, 1))
    same_csc(dc[:], ref)
    same_csc(dc, ref, "the input is unchanged")


@pytest.mark.parametrize("with_targets", [True, False])
def test_stacks(with_targets):
    """three parts either way; d > n and n > d for the pointer length of vstack (tensor/sparse.nim:598)"""
    v, h = K.stack_parts(with_targets)
    cv, ch = [R.to_csc(X) for X in v], [R.to_csc(X) for X in h]
    dv, dh = [up_csc(c) for c in cv], [up_csc(c) for c in ch]
    V, H = nf.vstack(*dv), nf.hstack(dh)
    same_csc(V, R.vstack(cv), "vstack")
    same_csc(H, R.hstack(ch), "hstack")
    same_csr(nf.toCSRDataset(V), R.to_csr(R.vstack(cv)))
    same_csr(nf.toCSRDataset(H), R.to_csr(R.hstack(ch)))
    for name in ("wide", "tall"):
        c = R.to_csc(ALL[name])
        d2 = nf.vstack(up_csc(c), up_csc(c))
        same_csc(d2, R.vstack([c, c]), name)
        assert len(d2.to_host()[0]) == c.d + 1
    same_csc(nf.vstack(dv[0]), cv[0], "one part")
    for dsx, c in zip(dv, cv):
        same_csc(dsx, c, "the inputs are unchanged")


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("axis", [0, 1])
def test_normalize(axis, norm):
    for name in ("literal", "unsorted_rows", "long", "dense", "repeat_in_row", "no_entries", "one_column"):
        ref = R.to_csc(ALL[name])
        dc = up_csc(ref)
        assert nf.normalize(dc, axis=axis, norm=norm) is None
        want = R.normalize(ref, axis, norm)
        same_csc(dc, want, "%s axis %d %s" % (name, axis, norm))
        same_csr(nf.toCSRDataset(dc), R.to_csr(want), name)


def test_loaders_as_csc(tmp_path):
    X = ALL["unsorted_rows"]
    text = KK.svmlight_text(X)
    p = tmp_path / "x.svm"
    p.write_text(text)
    rows, _ = nf.parseText(text)
    ri, rx, rd, _ = rows.to_host()
    parsed = RR.Csr(ri, rx, rd, rows.nSamples, rows.nFeatures, y=rows.targets())
    for ds, y in (nf.loadSVMLightFile(str(p), layout="csc"), nf.parseText(text, layout="csc"),
                  nf.loadSVMLightFile(str(p), nFeatures=X.d + 3, layout="csc")):
        want = R.to_csc(RR.Csr(ri, rx, rd, rows.nSamples, ds.nFeatures, y=parsed.y))
        same_csc(ds, want)
        assert np.array_equal(y, np.array(X.y))
    assert nf.loadSVMLightFile(str(p), nFeatures=X.d + 3, layout="csc")[0].nFeatures == X.d + 3
    with pytest.raises(ValueError, match="nFeatures is 2 but dataset has at least"):
        nf.loadSVMLightFile(str(p), nFeatures=2, layout="csc")
    with pytest.raises(ValueError, match="layout"):
        nf.loadSVMLightFile(str(p), layout="coo")
    for name, (text, kept, csr_refuses) in K.RATING_TEXTS.items():
        q = tmp_path / (name + ".txt")
        q.write_text(text)
        want = R.load_user_item_csc(text)
        assert want.n == kept
        for ds, y in (nf.loadUserItemRatingFile(str(q), layout="csc"), nf.parseUserItemRatingText(text, layout="csc")):
            same_csc(ds, want, name)
            assert np.array_equal(y, np.array(want.y))
        if csr_refuses:  # the four-character line: skipped as CSC, refused as CSR
            with pytest.raises(ValueError, match="malformed"):
                nf.loadUserItemRatingFile(str(q))
            with pytest.raises(ValueError, match="malformed"):
                nf.parseUserItemRatingText(text, layout="csr")
        else:
            same_csr(nf.loadUserItemRatingFile(str(q))[0], RR.load_user_item(text), name)


def test_beyond_one_pass_of_every_launch():
    """600000 rows of 0 to 3 entries, about 900000 entries: more than one pass of the element-wise kernels (524288 elements on
    256 CUs), of the kernels with 8 lanes per segment (65536 segments) and of those with a wavefront per segment (8192: the
    50 columns average 18000 entries).  Both transpositions, the slice and vstack, against vectorised numpy (a stable argsort
    is the reference's append order)."""
    rng = np.random.default_rng(2540)
    n, d = 600000, 50
    lens = rng.integers(0, 4, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(I64)
    nnz = int(indptr[-1])
    assert nnz > 524288
    indices = rng.integers(0, d, nnz).astype(I64)  # a row may repeat an id: the stable order shows
    data = rng.uniform(-2, 2, nnz)
    y = rng.standard_normal(n)
    row_of = np.repeat(np.arange(n), lens)
    ds = nf.newCSRDataset(data, indices, indptr, n, d)
    ds.set_targets(y)

    def csc_of(rows, cols, vals, d_):
        order = np.argsort(cols, kind="stable")
        return np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=d_))]).astype(I64), rows[order], vals[order]

    dc = nf.toCSCDataset(ds)
    cp, ci, cd = csc_of(row_of, indices, data, d)
    gp, gi, gd = dc.to_host()
    assert np.array_equal(gp, cp) and np.array_equal(gi, ci) and np.array_equal(gd, cd) and np.array_equal(dc.targets(), y)
    # back: rows stably sorted by column id
    col_of = np.repeat(np.arange(d), np.diff(cp))
    rp, rj, rv = csc_of(col_of, ci, cd, n)
    back = nf.toCSRDataset(dc)
    bp, bi, bd, _ = back.to_host()
    assert np.array_equal(bp, rp) and np.array_equal(bi, rj) and np.array_equal(bd, rv) and np.array_equal(back.targets(), y)
    # the slice [n/4, 3n/4)
    a, b = n // 4, 3 * n // 4
    keep = (ci >= a) & (ci < b)
    sl = dc[a:b]
    sp, si, sd = sl.to_host()
    want_p = np.concatenate([[0], np.cumsum(np.bincount(col_of[keep], minlength=d))]).astype(I64)
    assert sl.shape == [b - a, d] and np.array_equal(sp, want_p) and np.array_equal(si, ci[keep] - a) and np.array_equal(sd, cd[keep])
    assert np.array_equal(sl.targets(), y[a:b])
    # vstack of the CSC with itself: per column the part's column twice, the second with ids offset by n
    v = nf.vstack(dc, dc)
    vp, vi, vd = v.to_host()
    two = np.concatenate([col_of * 2, col_of * 2 + 1])
    order = np.argsort(two, kind="stable")
    assert v.shape == [2 * n, d] and np.array_equal(vp, 2 * cp)
    assert np.array_equal(vi, np.concatenate([ci, ci + n])[order]) and np.array_equal(vd, np.tile(cd, 2)[order])
    assert np.array_equal(v.targets(), np.tile(y, 2))


# ---- consumers of rows run on the twin ----
def _fm(d, degree, fitLower, task="regression"):
    rng = np.random.default_rng(90 + degree)
    fm = nf.newFactorizationMachine(task, degree=degree, nComponents=4, fitLower=fitLower, warmStart=True)
    fm.set_params(rng.standard_normal((fm.nOrders, 4, d + fm.nAugments)) * 0.3, rng.standard_normal(d) * 0.3, 0.25)
    return fm


def _same_predictions(model, dc, dr, y):
    a, b = model.decisionFunction(dc), model.decisionFunction(dr)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and np.abs(a).max() > 0
    assert model.predict(dc).tobytes() == model.predict(dr).tobytes()
    assert model.score(dc, y) == model.score(dr, y)
    ma, mb = model.metrics(dc, y), model.metrics(dr, y)
    assert sorted(ma) == sorted(mb) and all(np.array_equal(ma[k], mb[k], equal_nan=True) for k in ma)
    return a


@pytest.mark.parametrize("name", ["long", "repeat_in_row", "unsorted_rows"])
def test_predictions_are_the_row_twins(name):
    """decisionFunction / predict / score / metrics of a CSCDataset are bit-equal to those of toCSRDataset of it: FM of degree 2
    and 3 with fitLower = augment, explicit lower orders, and the convex model in both kernels"""
    X = ALL[name]
    dc = nf.toCSCDataset(up(X))
    dr = nf.toCSRDataset(dc)
    y = np.array(X.y)
    for degree, lower in ((2, "augment"), (3, "augment"), (3, "explicit")):
        got = _same_predictions(_fm(X.d, degree, lower), dc, dr, y)
        if degree == 2 and name != "repeat_in_row":  # and they are the predictions of the matrix itself
            assert np.allclose(got, _fm(X.d, degree, lower).decisionFunction(up(X)), rtol=1e-10, atol=1e-12)
    fmc = _fm(X.d, 2, "augment", task="classification")
    _same_predictions(fmc, dc, dr, np.sign(y))
    assert fmc.predictProba(dc).tobytes() == fmc.predictProba(dr).tobytes()
    rng = np.random.default_rng(7)
    for ignoreDiag in (True, False):
        cfm = nf.newConvexFactorizationMachine("regression", maxComponents=4, ignoreDiag=ignoreDiag)
        cfm.set_params(rng.normal(size=(3, X.d)), np.array([0.5, -1.5, 2.0]), rng.normal(size=X.d), 0.25)
        _same_predictions(cfm, dc, dr, y)


def _solver(kind):
    kw = dict(maxIter=2, verbose=0, tol=0)
    return {"cd": lambda: nf.newCD(**kw), "pcd": lambda: nf.newPCD(reg=nf.newL1(), **kw), "pbcd": lambda: nf.newPBCD(reg=nf.newL21(), **kw),
            "hazan": lambda: nf.newHazan(**kw), "gcd": lambda: nf.newGreedyCD(**kw)}[kind]()


def _start(d):
    return np.random.default_rng(5).standard_normal(d)


@pytest.mark.parametrize("kind", ["cd", "pcd", "pbcd", "hazan", "gcd"])
def test_column_solvers_fit_a_csc_dataset(kind):
    """two iterations on n = 80, d = 8, k = 4: the parameters after fit(Xcsc) are byte-equal to fit(toCSRDataset(Xcsc))"""
    X = K.trainable_case()
    y = np.array(X.y)
    convex = kind in ("hazan", "gcd")
    out = []
    for layout in ("csc", "csr"):
        dc = nf.toCSCDataset(up(X))
        ds = dc if layout == "csc" else nf.toCSRDataset(dc)
        if convex:
            m = nf.newConvexFactorizationMachine("regression", maxComponents=4)
            _solver(kind).fit(ds, y, m, powerInit=_start)
            out.append((m.P.copy(), m.lams.copy(), m.w.copy(), m.intercept))
        else:
            m = _fm(X.d, 2, "explicit")
            opt = _solver(kind)
            if layout == "csc":
                m.init(ds)
                assert opt.schedule(ds, m) == opt.schedule(nf.toCSRDataset(dc), m)
            opt.fit(ds, y, m)
            out.append((m.P.copy(), m.w.copy(), m.intercept))
    for a, b in zip(*out):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.isfinite(out[0][0]).all()
    if not convex:
        assert not np.array_equal(out[0][0], _fm(X.d, 2, "explicit").P)


def test_a_repeated_pair_predicts_but_does_not_train():
    indptr, indices, data, n, d = K.repeat_in_column_csc()
    dc = nf.newCSCDataset(np.array(data), np.array(indices, dtype=I64), np.array(indptr, dtype=I64), n, d)
    fm = _fm(d, 2, "explicit")
    assert fm.decisionFunction(dc).tobytes() == fm.decisionFunction(nf.toCSRDataset(dc)).tobytes()
    with pytest.raises(nf.NfmError, match="distinct"):
        nf.newCD(maxIter=1, verbose=0, tol=0).fit(dc, np.zeros(n), fm)


# ---- refusals ----
def _rc(fn, *args):
    rc = fn(*args)
    return rc, capi.lib().nfm_last_error().decode()


def test_refusals_of_the_hosts(tmp_path):
    X = K.trainable_case()
    dc, ds = nf.toCSCDataset(up(X)), up(X)
    y = np.array(X.y)
    kw = dict(maxIter=1, verbose=0, tol=0)
    row_wise = [nf.newSGD(**kw), nf.newAdaGrad(**kw), nf.newMBPSGD(reg=nf.newL1(), **kw), nf.newPSGD(reg=nf.newL1(), **kw),
                nf.newPGD(reg=nf.newL1(), **kw), nf.newFISTA(reg=nf.newL1(), **kw), nf.newNMAPGD(reg=nf.newL1(), **kw),
                nf.newKatyusha(reg=nf.newL1(), **kw)]
    for opt in row_wise:
        with pytest.raises(ValueError, match="toCSRDataset"):
            opt.fit(dc, y, _fm(X.d, 2, "explicit"))
    with pytest.raises(ValueError, match="toCSRDataset"):
        nf.newSGD(mode="minibatch", **kw).fit(dc, y, _fm(X.d, 2, "explicit"), devices=[0, 0])
    with pytest.raises(ValueError, match="toCSRDataset"):
        nf.predictAllWithGrad(dc, y, _fm(X.d, 2, "explicit"))
    for call in (lambda: nf.dumpSVMLightFile(str(tmp_path / "x.svm"), dc, y), lambda: nf.formatText(dc), lambda: dc[[0, 1]],
                 lambda: dc[np.array([2, 1])], lambda: nf.shuffle(dc, y), lambda: nf.shuffle(dc, y, [1, 0])):
        with pytest.raises(ValueError, match="toCSRDataset"):
            call()
    with pytest.raises(ValueError, match="not supported for CSCMatrix"):
        dc[[0, 1]]
    for stack in (nf.vstack, nf.hstack):
        with pytest.raises(ValueError, match="cannot be stacked together"):
            stack(dc, ds)
    other = nf.Context(0)
    try:
        far = nf.toCSCDataset(nf.newCSRDataset(np.array(X.data), np.array(X.indices, dtype=I64), np.array(X.indptr, dtype=I64), X.n, X.d, ctx=other))
        with pytest.raises(ValueError, match="different contexts"):
            nf.vstack(dc, far)
        del far
    finally:
        other.close()
    F = KK.field_case(2303, 40, 30, 3)
    df = nf.newCSRFieldDataset(np.array(F.data), np.array(F.indices, dtype=I64), np.array(F.indptr, dtype=I64), np.array(F.fields, dtype=I64),
                               F.n, F.d, F.n_fields)
    with pytest.raises(ValueError, match="field-aware"):
        nf.toCSCDataset(df)
    with pytest.raises(ValueError, match=r"shape\[1\]\.$"):
        nf.vstack(dc, nf.toCSCDataset(up(ALL["tall"])))
    with pytest.raises(ValueError, match=r"shape\[0\]$"):
        nf.hstack(dc, nf.toCSCDataset(up(ALL["tall"])))
    for bad in ((2, 2), (0, X.n + 1), (-1, 1)):
        with pytest.raises(ValueError, match="indicesRow|nSamples < 1"):
            dc[bad[0]:bad[1]]
    with pytest.raises(ValueError, match="sample index 80 out of range"):
        nf.newCSCDataset(np.ones(1), np.array([80], dtype=I64), np.array([0, 1] + [1] * 7, dtype=I64), 80, 8)
    with pytest.raises(ValueError, match="non-decreasing"):
        nf.newCSCDataset(np.ones(2), np.array([0, 1], dtype=I64), np.array([0, 2, 1, 2], dtype=I64), 4, 3)


def test_refusals_of_the_c_abi(tmp_path):
    L = capi.lib()
    X = K.trainable_case()
    dc, ds = nf.toCSCDataset(up(X)), up(X)
    dc.set_targets(np.array(X.y))
    h = C.c_void_p()
    lay = C.c_int32(-1)
    assert L.nfm_dataset_layout(dc.h, C.byref(lay)) == 0 and lay.value == capi.LAYOUT["csc"]
    assert L.nfm_dataset_layout(ds.h, C.byref(lay)) == 0 and lay.value == capi.LAYOUT["csr"]
    rows = np.array([0, 1], dtype=I64)
    n = C.c_int64(0)
    unsupported = [
        (L.nfm_dataset_select_rows, dc.h, rows.ctypes.data_as(C.c_void_p), 2, C.byref(h)),
        (L.nfm_dataset_dump_svmlight, dc.h, str(tmp_path / "x.svm").encode(), None, 0, 0),
        (L.nfm_dataset_format_text, dc.h, None, 0, 0, None, 0, C.byref(n)),
    ]
    for fn, *args in unsupported:
        rc, msg = _rc(fn, *args)
        assert rc == capi.ERR_UNSUPPORTED and "nfm_dataset_to_csr" in msg and "toCSRDataset" in msg, (fn.__name__, rc, msg)
    # the row-wise solvers, at their epoch / begin_fit entries
    kw = dict(maxIter=1, verbose=0, tol=0)
    fm = _fm(X.d, 2, "explicit")
    zero, one = C.c_double(0), C.c_double(0)
    for opt, mode in ((nf.newSGD(**kw), "sequential"), (nf.newAdaGrad(**kw), "sequential"), (nf.newMBPSGD(reg=nf.newL1(), **kw), "minibatch"),
                      (nf.newPSGD(reg=nf.newL1(), **kw), "sequential")):
        oh = opt._handle(fm, dc.ctx, mode)
        rc, msg = _rc(L.nfm_psgd_begin_fit if isinstance(opt, nf.PSGD) else L.nfm_opt_epoch,
                      *((oh, dc.h) if isinstance(opt, nf.PSGD) else (oh, dc.h, None, 0, X.n, C.byref(zero), C.byref(one))))
        assert rc == capi.ERR_UNSUPPORTED and "nfm_dataset_to_csr" in msg, (type(opt).__name__, rc, msg)
    for opt, begin in ((nf.newPGD(reg=nf.newL1(), **kw), lambda oh: L.nfm_pgd_begin_fit(oh, dc.h, 0)),
                       (nf.newKatyusha(reg=nf.newL1(), **kw), lambda oh: L.nfm_katyusha_begin_fit(oh, dc.h))):
        opt._resolve(ds, fm)
        oh = opt._handle(fm, dc.ctx)
        rc = begin(oh)
        msg = L.nfm_last_error().decode()
        assert rc == capi.ERR_UNSUPPORTED and "nfm_dataset_to_csr" in msg, (type(opt).__name__, rc, msg)
    # mixed layouts, and the column getter of a row-major dataset
    hs = (C.c_void_p * 2)(dc.h, ds.h)
    for fn in (L.nfm_dataset_vstack, L.nfm_dataset_hstack):
        rc, msg = _rc(fn, hs, 2, C.byref(h))
        assert rc == capi.ERR_INVALID and "cannot be stacked together" in msg
    assert _rc(L.nfm_dataset_get_csc, ds.h, None, None, None)[0] == capi.ERR_INVALID
    # a field-aware dataset, too many samples
    F = KK.field_case(2303, 40, 30, 3)
    df = nf.newCSRFieldDataset(np.array(F.data), np.array(F.indices, dtype=I64), np.array(F.indptr, dtype=I64), np.array(F.fields, dtype=I64),
                               F.n, F.d, F.n_fields)
    rc, msg = _rc(L.nfm_dataset_to_csc, df.h, C.byref(h))
    assert rc == capi.ERR_UNSUPPORTED and "field-aware" in msg
    ip = np.zeros(2, dtype=I64)
    rc, msg = _rc(L.nfm_dataset_create_csc, dc.ctx.h, 2 ** 31, 1, ip.ctypes.data_as(C.c_void_p), None, None, None, C.byref(h))
    assert rc == capi.ERR_UNSUPPORTED and "int32" in msg
    rc, msg = _rc(L.nfm_dataset_create_csc_device, dc.ctx.h, 2 ** 31, 1, 0, 1, None, None, None, C.byref(h))
    assert rc == capi.ERR_UNSUPPORTED and "int32" in msg
