"""-m gpu: datasets made from datasets on the device (nimfm_amd/csrc/dataset_ops.hip) against the
plain-Python restatement of the reference's procs (tests/dataset_ops_restatement.py), bit for bit: np.array_equal on
to_host(), targets(), shape and nFields of every result.  The cases are tests/dataset_ops_cases.py's;
tests/test_dataset_ops_restatement.py holds the restatement to dense numpy and pins what the cases contain.

Nothing here has a tolerance: the ops are copies and in-order folds (x + y*y, sqrt, x + |y|, max, one division per entry,
each rounded once, no fused multiply-add), so the device's bits are the restatement's."""
import ctypes as C

import numpy as np
import pytest

import dataset_ops_cases as K
import dataset_ops_restatement as R
import nimfm_amd as nf
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
NORMS = ("l1", "l2", "linfty")


def up(X):
    """a restatement matrix uploaded from the host"""
    if X.fields is None:
        ds = nf.newCSRDataset(np.array(X.data), np.array(X.indices, dtype=np.int64), np.array(X.indptr, dtype=np.int64), X.n, X.d)
    else:
        ds = nf.newCSRFieldDataset(np.array(X.data), np.array(X.indices, dtype=np.int64), np.array(X.indptr, dtype=np.int64),
                                   np.array(X.fields, dtype=np.int64), X.n, X.d, X.n_fields)
    if X.y is not None:
        ds.set_targets(np.array(X.y))
    return ds


def down(ds, with_y=True):
    """a device dataset as a restatement matrix"""
    indptr, indices, data, fields = ds.to_host()
    return R.Csr(indptr, indices, data, ds.nSamples, ds.nFeatures, fields, ds.nFields, ds.targets() if with_y else None)


def same(ds, ref, what=""):
    indptr, indices, data, fields = ds.to_host()
    assert ds.shape == [ref.n, ref.d] and ds.nFields == ref.n_fields and ds.nnz == ref.nnz, what
    assert np.array_equal(indptr, np.array(ref.indptr, dtype=np.int64)), what
    assert np.array_equal(indices, np.array(ref.indices, dtype=np.int64)), what
    assert np.array_equal(data, np.array(ref.data, dtype=np.float64), equal_nan=True), what
    assert (fields is None) == (ref.fields is None), what
    if fields is not None:
        assert np.array_equal(fields, np.array(ref.fields, dtype=np.int64)), what
    if ref.y is None:
        with pytest.raises(ValueError, match="no targets"):
            ds.targets()
    else:
        assert np.array_equal(ds.targets(), np.array(ref.y)), what


@pytest.fixture(scope="module")
def cases():
    X, S = K.main_case(), K.side_case()
    F3, F5, F4 = K.field_cases()
    return dict(X=X, S=S, F3=F3, F5=F5, F4=F4, dX=up(X), dS=up(S), dF3=up(F3), dF5=up(F5), dF4=up(F4))


@pytest.fixture(scope="module")
def parsed(cases):
    """the main case through the text loader: another maker of device datasets (its arrays come from ingest.hip)"""
    ds, _ = nf.parseText(K.svmlight_text(cases["X"]))
    return ds, down(ds)


def test_select_rows_and_slices(cases, parsed):
    for ds, X in ((cases["dX"], cases["X"]), parsed):
        for name, rows in K.selections().items():
            same(ds[rows], R.select_rows(X, rows), name)
            same(ds[np.array(rows, dtype=np.int32)], R.select_rows(X, rows), name)
        for a, b in K.SLICES:
            same(ds[a:b], R.slice_rows(X, a, b), "slice %d:%d" % (a, b))
        same(ds[range(3, 9)], R.slice_rows(X, 3, 9))
        same(ds[:5], R.slice_rows(X, 0, 5))
        same(ds[290:], R.slice_rows(X, 290, X.n))
        same(ds, X, "the input is unchanged")
    assert cases["dX"][K.selections()["zero_entries"]].nnz == 0


def test_field_aware_select_and_stacks(cases):
    F3, F5, F4, dF3, dF5, dF4 = (cases[k] for k in ("F3", "F5", "F4", "dF3", "dF5", "dF4"))
    rows = [7, 7, 0, 39, 12]
    same(dF5[rows], R.select_rows(F5, rows))
    same(dF5[4:30], R.slice_rows(F5, 4, 30))
    same(nf.vstack(dF3, dF5), R.vstack([F3, F5]))
    same(nf.vstack(dF5, dF3, dF4), R.vstack([F5, F3, F4]), "n_fields = max, no targets: one part has none")
    same(nf.hstack(dF3, dF5), R.hstack([F3, F5]), "fields offset by the parts before")
    same(nf.hstack([dF5, dF3, dF5]), R.hstack([F5, F3, F5]))
    for ds, X in ((dF3, F3), (dF5, F5), (dF4, F4)):
        same(ds, X, "the input is unchanged")


def test_plain_stacks(cases, parsed):
    X, S, dX, dS = cases["X"], cases["S"], cases["dX"], cases["dS"]
    same(nf.vstack(dX, dX[3:9], dX), R.vstack([X, R.slice_rows(X, 3, 9), X]))
    same(nf.vstack(dX), R.vstack([X]))
    same(nf.hstack(dX, dS), R.hstack([X, S]), "a part's row empty where the other's is not")
    same(nf.hstack(dS, dX, dS), R.hstack([S, X, S]))
    # parts whose rows average 64 entries or more: the copy kernel takes a wavefront per row
    rows = K.selections()["long_rows"]
    same(nf.hstack(dX[rows], dS[rows], dX[rows]), R.hstack([R.select_rows(X, rows), R.select_rows(S, rows), R.select_rows(X, rows)]))
    # a part without targets: vstack has none, hstack takes the first part's
    bare = nf.newCSRDataset(np.array(S.data), np.array(S.indices), np.array(S.indptr), S.n, S.d)
    Sb = R.Csr(S.indptr, S.indices, S.data, S.n, S.d)
    same(nf.vstack(dS, bare), R.vstack([S, Sb]))
    same(nf.hstack(dX, bare), R.hstack([X, Sb]))
    same(nf.hstack(bare, dX), R.hstack([Sb, X]))
    # parts made by different makers
    pds, P = parsed
    same(nf.vstack(pds, pds[5:6]), R.vstack([P, R.slice_rows(P, 5, 6)]))
    same(nf.hstack(pds, dS), R.hstack([P, S]))
    for ds, Y in ((dX, X), (dS, S), (pds, P)):
        same(ds, Y, "the input is unchanged")


@pytest.mark.parametrize("norm", NORMS)
def test_normalize(cases, parsed, norm):
    """both axes on the main case (a repeated id in a row: its column's entries still add up in storage order; a row and
    a column of zero norm; a column in 90 rows: more than one 8-lane round, and more than a wavefront's worth), on the
    parsed copy and on a field-aware one.  normalize works in place, as the reference's: the object keeps working after the
    handle swap -- decisionFunction on it, then a second normalize."""
    for X in (cases["X"], parsed[1], cases["F5"]):
        for axis in (1, 0):
            ds = up(X)
            assert nf.normalize(ds, axis=axis, norm=norm) is None
            once = R.normalize(X, axis, norm)
            same(ds, once, "axis %d" % axis)
            if X.fields is None:
                fm = nf.newFactorizationMachine("regression", nComponents=3, warmStart=True)
                rng = np.random.default_rng(5)
                fm.set_params(rng.standard_normal((1, 3, X.d)) * 0.1, rng.standard_normal(X.d) * 0.1, 0.25)
                assert np.array_equal(fm.decisionFunction(ds), fm.decisionFunction(up(once)))
            nf.normalize(ds, axis=1 - axis, norm=norm)
            same(ds, R.normalize(once, 1 - axis, norm), "axis %d then %d" % (axis, 1 - axis))
    same(cases["dX"], cases["X"], "the input is unchanged")
    with pytest.raises(ValueError, match="axis must be 0 or 1"):
        nf.normalize(up(cases["S"]), axis=2)
    with pytest.raises(ValueError, match="norm must be one of"):
        nf.normalize(up(cases["S"]), norm="l3")


def test_shuffle(cases):
    X, dX = cases["X"], cases["dX"]
    y = np.array(X.y) * 2.0  # the host's y, not the dataset's targets
    idx = K.selections()["random_80_percent"]
    Xs, ys = nf.shuffle(dX, y, idx)
    same(Xs, R.select_rows(X, idx))
    assert np.array_equal(ys, y[idx])
    # the drawn permutation: the forward draw from the global generator
    nf.randomize(11)
    Xs, ys = nf.shuffle(dX, y)
    perm = np.arange(X.n, dtype=np.int64)
    nf.NimRand(11).shuffleForward(perm)
    assert sorted(perm.tolist()) == list(range(X.n)) and not np.array_equal(perm, np.arange(X.n))
    same(Xs, R.select_rows(X, perm.tolist()))
    assert np.array_equal(ys, y[perm])
    # the procedure (dataset.nim:388-394) with the generator's draws replayed: j = position of perm[i] among the not yet placed
    left, js = list(range(X.n)), []
    for i in range(X.n):
        j = left.index(perm[i], i) - i
        js.append(j)
        left[i], left[i + j] = left[i + j], left[i]
    assert all(0 <= j <= X.n - 1 - i for i, j in enumerate(js))
    it = iter(js)
    assert R.forward_draw(X.n, lambda mx: next(it)) == perm.tolist()
    with pytest.raises(ValueError) as e:
        nf.shuffle(dX, y[:-1])
    assert str(e.value) == "X.nSamples != len(y)"


def test_error_texts(cases, tmp_path):
    dX, dS, dF3 = cases["dX"], cases["dS"], cases["dF3"]
    L = capi.lib()
    h = C.c_void_p()

    def abi(rc, text):
        assert rc == capi.ERR_INVALID and L.nfm_last_error().decode() == text

    for rows, text in (([], "Invalid slice: nSamples < 1."), ([0, 300], "max(indicesRow) 300 >= 300."), ([2, -1], "min(indicesRow) -1 < 0.")):
        with pytest.raises(ValueError) as e:
            dX[rows]
        assert str(e.value) == text
        r = np.array(rows, dtype=np.int64)
        abi(L.nfm_dataset_select_rows(dX.h, r.ctypes.data_as(C.c_void_p), len(r), C.byref(h)), text)
    for (a, b), text in (((4, 4), "Invalid slice: nSamples < 1."), ((7, 3), "Invalid slice: nSamples < 1."),
                         ((290, 301), "max(indicesRow) 300 >= 300."), ((-2, 5), "min(indicesRow) -2 < 0.")):
        with pytest.raises(ValueError) as e:
            dX[a:b]
        assert str(e.value) == text
        abi(L.nfm_dataset_slice_rows(dX.h, a, b, C.byref(h)), text)
    with pytest.raises(ValueError, match="step 1"):
        dX[0:10:2]
    with pytest.raises(TypeError):
        dX[[0.5, 1.0]]
    pair = (C.c_void_p * 2)(dX.h, dS.h)
    with pytest.raises(ValueError) as e:
        nf.vstack(dX, dS)
    assert str(e.value) == "All matrics must have the same shape[1]."
    abi(L.nfm_dataset_vstack(pair, 2, C.byref(h)), "All matrics must have the same shape[1].")
    with pytest.raises(ValueError) as e:
        nf.hstack(dX, dS[0:10])
    assert str(e.value) == "All matrics must have the same shape[0]."
    short = dS[0:10]
    pair = (C.c_void_p * 2)(dX.h, short.h)
    abi(L.nfm_dataset_hstack(pair, 2, C.byref(h)), "All matrics must have the same shape[0].")
    with pytest.raises(ValueError, match="plain and field-aware"):
        nf.vstack(dX, dF3)
    with pytest.raises(ValueError, match="at least one"):
        nf.hstack()
    # the summed n_features must fit as nfm_dataset_create_csr's must
    wide = nf.newCSRDataset(np.ones(1), np.array([5]), np.array([0, 1]), 1, 2**30)
    with pytest.raises(nf.NfmError, match="n_features must fit int32"):
        nf.hstack(wide, wide)
    assert L.nfm_dataset_normalize(dX.h, 3, 0, C.byref(h)) == capi.ERR_INVALID
    assert L.nfm_dataset_normalize(dX.h, 1, 3, C.byref(h)) == capi.ERR_INVALID
    # a dataset used in row blocks is not resident: refused by the hosts
    nf.convertSVMLightFile(_write(tmp_path / "s.svm", "1 1:1 3:2\n-1 2:1\n1 1:3\n"), str(tmp_path / "sx"), str(tmp_path / "sy"))
    st, ys = nf.newStreamCSRDataset(str(tmp_path / "sx"), str(tmp_path / "sy"), cacheRows=2)
    for call in (lambda: nf.shuffle(st, ys), lambda: nf.vstack(st, st), lambda: nf.hstack(st), lambda: nf.normalize(st)):
        with pytest.raises(ValueError, match="resident on the device"):
            call()
    same(dX, cases["X"], "the input is unchanged")


def _write(path, text):
    path.write_bytes(text.encode())
    return str(path)


@pytest.mark.parametrize("name,text,bad", K.RATING_TEXTS, ids=[t[0] for t in K.RATING_TEXTS])
def test_rating_loader(name, text, bad, tmp_path):
    L = capi.lib()
    if bad:
        with pytest.raises(ValueError):
            nf.parseUserItemRatingText(text)
        h = C.c_void_p()
        assert L.nfm_dataset_parse_user_item(nf.default_context().h, text.encode(), len(text), C.byref(h)) == capi.ERR_INVALID
        with pytest.raises(ValueError):
            nf.loadUserItemRatingFile(_write(tmp_path / "r.txt", text))
        return
    want = R.load_user_item(text)
    ds, y = nf.parseUserItemRatingText(text)
    same(ds, want, name)
    assert np.array_equal(y, np.array(want.y))
    ds, y = nf.loadUserItemRatingFile(_write(tmp_path / "r.txt", text))
    same(ds, want, name + " (file)")
    assert ds.ingest_stats()[0] == len(text)


def test_rating_loader_ids_that_do_not_fit():
    with pytest.raises(ValueError, match="do not fit int32"):
        nf.parseUserItemRatingText("1 1 5\n3000000000 2 1\n")
    with pytest.raises(ValueError, match="malformed"):
        nf.parseUserItemRatingText("1 1 5\n1234567890123456789012 2 1\n")
    with pytest.raises(ValueError, match="cannot be read"):
        nf.loadUserItemRatingFile("/nonexistent/ratings.txt")


def test_beyond_one_pass_of_every_launch():
    """Launch geometry (dataset_ops.hip): every kernel walks its work in a grid-stride loop over at most n_cu * 8 workgroups
    of 256 threads -- on 256 CUs 524288 elements per pass of the element-wise kernels (row lengths, the plain copies, the
    indptr shift of vstack, the cursor advance of hstack, the per-line and per-row kernels of the rating loader) and 65536 rows
    per pass of the kernels with 8 lanes per row (the copies of select and hstack for rows that average fewer than 64 entries,
    the row norm).  2000 rows of 0 to 3 entries selected 600000 times over give 600000 rows and about 900000 entries: more
    than one pass of each.  (The wavefront-per-row variants of the two copies run the same loop body with 8192 rows per pass;
    the "long_rows" selection covers their lane arithmetic.)  The expectations are vectorised numpy (the restatement's loops
    would take a minute here); rows of at most three entries keep the in-order fold explicit."""
    rng = np.random.default_rng(2310)
    n, d, m = 2000, 50, 600000
    lens = rng.integers(0, 4, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(d, k, replace=False)) for k in lens]).astype(np.int64)
    data = rng.uniform(-2, 2, len(indices))
    y = rng.standard_normal(n)
    ds = nf.newCSRDataset(data, indices, indptr, n, d)
    ds.set_targets(y)
    rows = rng.integers(0, n, m)
    # X[rows]
    olen = lens[rows]
    optr = np.concatenate([[0], np.cumsum(olen)]).astype(np.int64)
    nnz = int(optr[-1])
    assert m > 524288 and nnz > 524288
    orow = np.repeat(np.arange(m), olen)
    src = indptr[rows][orow] + (np.arange(nnz) - optr[orow])
    big = ds[rows]
    gp, gi, gd, _ = big.to_host()
    assert big.shape == [m, d] and np.array_equal(gp, optr) and np.array_equal(gi, indices[src]) and np.array_equal(gd, data[src])
    assert np.array_equal(big.targets(), y[rows])
    # vstack([big, big]) and hstack([big, big])
    v = nf.vstack(big, big)
    vp, vi, vd, _ = v.to_host()
    assert np.array_equal(vp, np.concatenate([optr, optr[1:] + nnz])) and np.array_equal(vi, np.tile(gi, 2))
    assert np.array_equal(vd, np.tile(gd, 2)) and np.array_equal(v.targets(), np.tile(y[rows], 2))
    hs = nf.hstack(big, big)
    hp, hi, hd, _ = hs.to_host()
    first = np.arange(nnz) + optr[orow]
    ei, ed = np.zeros(2 * nnz, dtype=np.int64), np.zeros(2 * nnz)
    ei[first], ei[first + olen[orow]] = gi, gi + d
    ed[first], ed[first + olen[orow]] = gd, gd
    assert hs.shape == [m, 2 * d] and np.array_equal(hp, 2 * optr) and np.array_equal(hi, ei) and np.array_equal(hd, ed)
    # normalize(axis=1, l2): ((0 + v0^2) + v1^2) + v2^2 in storage order, one rounding per operation
    val = np.zeros((m, 3))
    val[orow, np.arange(nnz) - optr[orow]] = gd
    nv = np.sqrt(((0.0 + val[:, 0] * val[:, 0]) + val[:, 1] * val[:, 1]) + val[:, 2] * val[:, 2])
    nf.normalize(big, axis=1, norm="l2")
    want = np.where(nv[orow] != 0.0, gd / np.where(nv[orow] != 0.0, nv[orow], 1.0), gd)
    assert np.array_equal(big.to_host()[2], want)
    # the rating loader: one thread per line, 600000 lines
    users, items, stars = rng.integers(1, 5000, m), rng.integers(0, 3000, m), rng.integers(1, 6, m)
    users[0], items[0] = 1, 0
    text = "".join("%d::%d::%d\n" % t for t in zip(users.tolist(), items.tolist(), stars.tolist()))
    rt, ry = nf.parseUserItemRatingText(text)
    nu = int(users.max())  # minUser = 1, minItem = 0
    rp, ri, rd, _ = rt.to_host()
    assert rt.shape == [m, nu + int(items.max()) + 1] and np.array_equal(rp, 2 * np.arange(m + 1)) and np.array_equal(rd, np.ones(2 * m))
    assert np.array_equal(ri[0::2], users - 1) and np.array_equal(ri[1::2], nu + items) and np.array_equal(ry, stars.astype(np.float64))


def _model(d):
    rng = np.random.default_rng(77)
    fm = nf.newFactorizationMachine("regression", nComponents=4, warmStart=True)
    fm.set_params(rng.standard_normal((1, 4, d)) * 0.03, rng.standard_normal(d) * 0.03, 0.5)
    return fm


def _fit(X, y, d):
    fm = _model(d)
    # (a step and a start small enough for the 200-entry row: finite on the CPU oracle for every matrix fitted here)
    nf.newSGD(maxIter=2, eta0=5e-4, verbose=0, tol=0, shuffle=False, mode="sequential").fit(X, y, fm)
    return fm


def test_device_made_datasets_train_as_uploaded_ones(cases):
    """max_row, repeats and the arrays of a device-made dataset are what an upload of the same matrix gets: a model fitted
    (SGD, the reference's order, two epochs) on either is the same, bit for bit.  The selections hold the 200-entry row, so
    a max_row taken from anything but the selected rows would show (the kernels size their per-sample scratch by it)."""
    X, S, dX, dS = cases["X"], cases["S"], cases["dX"], cases["dS"]
    rows = K.selections()["trainable"]
    T, dT = R.select_rows(X, rows), dX[rows]
    made = {
        "select": (dT, T),
        "slice": (dX[9:120], R.slice_rows(X, 9, 120)),
        "vstack": (nf.vstack(dT, dT[0:40]), R.vstack([T, R.slice_rows(T, 0, 40)])),
        "hstack": (nf.hstack(dT, dS[rows]), R.hstack([T, R.select_rows(S, rows)])),
    }
    for axis in (0, 1):
        dn = dX[rows]
        nf.normalize(dn, axis=axis, norm="l2")
        made["normalize axis %d" % axis] = (dn, R.normalize(T, axis, "l2"))
    for name, (ds, ref) in made.items():
        y = np.array(ref.y)
        a, b = _fit(ds, y, ref.d), _fit(up(ref), y, ref.d)
        assert np.array_equal(a.P, b.P) and np.array_equal(a.w, b.w) and a.intercept == b.intercept, name
        assert np.isfinite(a.P).all() and not np.array_equal(a.P, _model(ref.d).P), name


def test_a_selected_repeat_row_predicts_but_does_not_train(cases):
    X, dX = cases["X"], cases["dX"]
    rows = [K.ROW_1, K.ROW_REPEAT, K.ROW_64]
    ds, ref = dX[rows], R.select_rows(X, rows)
    fm = _fit(dX[[K.ROW_1, K.ROW_64, K.ROW_200]], np.array([0.5, -1.0, 2.0]), X.d)  # without that row: trains
    assert np.array_equal(fm.decisionFunction(ds), fm.decisionFunction(up(ref)))
    with pytest.raises(nf.NfmError, match="row 1"):
        nf.newSGD(maxIter=1, verbose=0, tol=0, shuffle=False, mode="sequential").fit(ds, np.array(ref.y), fm)
    for stacked in (nf.vstack(dX[0:3], ds), nf.hstack(ds, ds)):
        with pytest.raises(nf.NfmError, match="distinct"):
            nf.newSGD(maxIter=1, verbose=0, tol=0).fit(stacked, np.zeros(stacked.nSamples), _model(stacked.nFeatures))
