"""Datasets in HBM written as svmlight / libffm text by the device (nimfm_amd/csrc/dataset_text.hip, DESIGN.md section 24:
nfm_dataset_dump_svmlight, nfm_dataset_dump_ffm, nfm_dataset_format_text, nfm_format_f64) against oracle/ingest.py's
dump_svmlight / dump_ffm (the reference's dumpSVMLightFile / dumpFFMFile, dataset.nim:793-805, 825-837) and Python's repr.
Every comparison is byte equality."""
import ctypes as C
import hashlib
import os
import struct

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi
from nimfm_amd import host
from oracle import ingest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ["ingest_svm_1based.txt", "ingest_svm_0based.txt", "ingest_svm_digits.txt", "ingest_ffm_1based.txt",
         "ingest_ffm_0based.txt"]
MAX_D = 2147483647 - 64 - 1  # the largest n_features nfm_dataset_create_csr accepts


def upload(indptr, indices, data, y=None, fields=None, d=None, n_fields=None):
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float64)
    n = len(indptr) - 1
    if d is None:
        d = int(indices.max()) + 1 if len(indices) else 1
    if fields is None:
        ds = nf.newCSRDataset(data, indices, indptr, n, d)
    else:
        fields = np.asarray(fields, dtype=np.int64)
        if n_fields is None:
            n_fields = int(fields.max()) + 1 if len(fields) else 1
        ds = nf.newCSRFieldDataset(data, indices, indptr, fields, n, d, n_fields)
    if y is not None:
        ds.set_targets(np.asarray(y, dtype=np.float64))
    return ds


def oracle_text(indptr, indices, data, y, fields=None):
    if fields is None:
        return ingest.dump_svmlight(indptr, indices, data, y).encode()
    return ingest.dump_ffm(indptr, indices, fields, data, y).encode()


def first_difference(a, b):
    m = min(len(a), len(b))
    x, z = np.frombuffer(a, dtype=np.uint8, count=m), np.frombuffer(b, dtype=np.uint8, count=m)
    bad = np.nonzero(x != z)[0]
    at = int(bad[0]) if len(bad) else m
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), at, a[max(0, at - 30):at + 30], b[max(0, at - 30):at + 30])


def assert_same_text(got, want):
    assert got == want, first_difference(got, want)


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def special_values():
    """the hand-picked part of tests/test_format_num.py's corpus"""
    top = 0x7FEFFFFFFFFFFFFF
    b = [0, 1 << 63, 1, (1 << 52) - 1, 1 << 52, top, top | 1 << 63, 0x7FF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000]
    for e in range(-1074, 1024):
        c = bits_of(2.0 ** e)
        b += [v for v in (c - 1, c, c + 1) if 0 <= v <= top]
    for q in range(-323, 309):
        c = bits_of(float("1e%d" % q))
        b += [v for v in (c - 1, c, c + 1) if 0 <= v <= top]
    for x in (9999999999999998.0, 1e16, 0.0001, 9.999999999999999e-05, 123456.0, 9007199254740992.0, 1.2345678901234568e17,
              -2.2250738585072014e-308, 1e22, 1e23, 0.3, -1.5):
        b.append(bits_of(x))
    return np.array(b, dtype=np.uint64).view(np.float64)


# ---- 1. fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_fixtures(name):
    with open(os.path.join(GOLD, name), newline="") as f:
        text = f.read()
    ffm = "ffm" in name
    r = ingest.load_ffm(text) if ffm else ingest.load_svmlight(text)
    ds, _ = nf.parseText(text, withFields=ffm)
    want = oracle_text(r["indptr"], r["indices"], r["data"], r["y"], r["fields"] if ffm else None)
    assert_same_text(nf.formatText(ds), want)
    assert_same_text(nf.formatText(ds, chunkBytes=64), want)


# ---- 2. random matrices ------------------------------------------------------------------------------------------------
def random_csr(rng, n, d, density, ffm, n_fields=4):
    """tests/test_gpu_ingest.py::random_csr_text's construction, the arrays kept"""
    mask = rng.random((n, d)) < density
    mask[0, 0] = mask[n - 1, d - 1] = True
    rows, cols = np.nonzero(mask)
    data = rng.uniform(-1, 1, size=len(rows)) * 10.0 ** rng.integers(-8, 8, size=len(rows))
    indptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    y = rng.standard_normal(n)
    return indptr, cols.astype(np.int64), data, y, (cols % n_fields).astype(np.int64) if ffm else None


@pytest.fixture(scope="module", params=[(300, 120, 0.2, False), (300, 120, 0.2, True), (2000, 500, 0.02, False), (2000, 500, 0.02, True)],
                ids=["300x120", "300x120-ffm", "2000x500", "2000x500-ffm"])
def random_case(request):
    n, d, density, ffm = request.param
    indptr, cols, data, y, fields = random_csr(np.random.default_rng(24), n, d, density, ffm)
    return upload(indptr, cols, data, y, fields, d=d), oracle_text(indptr, cols, data, y, fields), ffm


def test_random_matrix_default_chunk(random_case, tmp_path):
    ds, want, ffm = random_case
    got = nf.formatText(ds)
    assert_same_text(got, want)
    p = str(tmp_path / "out.txt")
    (nf.dumpFFMFile if ffm else nf.dumpSVMLightFile)(p, ds)
    with open(p, "rb") as f:
        assert_same_text(f.read(), got)


@pytest.mark.parametrize("chunk", [64, 4096, "first row"])
def test_random_matrix_in_pieces(random_case, chunk, tmp_path):
    """64 bytes is less than most rows: one row per piece; "first row": a piece boundary exactly at a row boundary"""
    ds, want, ffm = random_case
    if chunk == "first row":
        chunk = want.index(b"\n")
    got = nf.formatText(ds, chunkBytes=chunk)
    assert_same_text(got, want)
    p = str(tmp_path / "out.txt")
    (nf.dumpFFMFile if ffm else nf.dumpSVMLightFile)(p, ds, chunkBytes=chunk)
    with open(p, "rb") as f:
        assert_same_text(f.read(), got)


# ---- 3. round trip on the device ---------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("ffm", [False, True])
def test_round_trip_on_the_device(ffm):
    vals = special_values()
    m = len(vals)
    per = 7
    n = (m + per - 1) // per
    indptr = np.minimum(np.arange(n + 1) * per, m).astype(np.int64)
    indices = (np.arange(m) * 13 % 1000).astype(np.int64)
    fields = (np.arange(m) % 5).astype(np.int64) if ffm else None
    y = vals[(np.arange(n) * 11) % m]
    ds = upload(indptr, indices, vals, y, fields, d=1000, n_fields=5)
    text = nf.formatText(ds, chunkBytes=100000)
    assert_same_text(text, oracle_text(indptr, indices, vals, y, fields))
    back, yb = nf.parseText(text, withFields=ffm, nFeatures=ds.nFeatures, nFields=ds.nFields if ffm else -1)
    gp, gi, gd, gf = back.to_host()
    assert back.nFeatures == 1000 and np.array_equal(gp, indptr) and np.array_equal(gi, indices)
    assert same_bits(gd, vals) and same_bits(yb, y)
    if ffm:
        assert back.nFields == 5 and np.array_equal(gf, fields)


# ---- 4. layout edges ---------------------------------------------------------------------------------------------------
def value_of_length(length, k):
    """a float64 whose text has `length` characters (3 .. 24)"""
    fixed = {3: "%d.0" % (1 + k % 9), 4: "%d.0" % (10 + k % 90), 5: "-%d.0" % (10 + k % 90), 23: "2.2250738585072014e-308",
             24: "-2.2250738585072014e-308", 22: "-1.234567890123456e+17", 21: "1.234567890123456e+17", 20: "-0.1234567890123456%d" % (1 + k % 9),
             19: "0.1234567890123456%d" % (1 + k % 9)}
    if length in fixed:
        t = fixed[length]
    else:  # 6 .. 18: "0." and length - 2 digits, the last one not 0
        t = "0." + "".join(str((k + i) % 9 + 1) for i in range(length - 2))
    v = float(t)
    assert len(repr(v)) == length, (length, t, repr(v))
    return v


def check(indptr, indices, data, y, fields=None, d=None, n_fields=None, chunks=(0, 64)):
    ds = upload(indptr, indices, data, y, fields, d=d, n_fields=n_fields)
    want = oracle_text(np.asarray(indptr), np.asarray(indices), np.asarray(data, dtype=np.float64), np.asarray(y, dtype=np.float64), fields)
    for c in chunks:
        assert_same_text(nf.formatText(ds, chunkBytes=c), want)
    return ds, want


def test_one_row_and_no_entries():
    check([0, 1], [0], [0.5], [1.0])
    check([0, 0], [], [], [-2.5])  # n = 1, nothing stored
    check([0, 0, 0, 0], [], [], [1.0, 2.0, 3.0])  # no entries at all
    check([0, 0, 0, 0], [], [], [1.0, 2.0, 3.0], fields=[])


def test_empty_rows_first_last_and_in_runs():
    lens = [0, 0, 3, 0, 0, 0, 1, 2, 0, 5, 0, 0]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(indptr[-1])
    check(indptr, np.arange(nnz) % 7, np.linspace(-1, 1, nnz), np.arange(len(lens)) * 0.5)
    # runs of empty rows longer than a workgroup's 256 items, around single entries
    lens = [0] * 700 + [1] + [0] * 300 + [2] + [0] * 513
    indptr = np.concatenate([[0], np.cumsum(lens)])
    check(indptr, [4, 1, 2], [0.25, -1e-7, 3e20], np.arange(len(lens)) % 3 - 1.0, chunks=(0, 1000))


def test_row_longer_than_a_span():
    rng = np.random.default_rng(5)
    lens = [1, 3000, 1, 1, 700, 1]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(indptr[-1])
    data = rng.uniform(-1, 1, nnz) * 10.0 ** rng.integers(-8, 8, nnz)
    for fields in (None, rng.integers(0, 3, nnz)):
        check(indptr, rng.integers(0, 5000, nnz), data, rng.standard_normal(len(lens)), fields=fields, d=5000, chunks=(0, 64, 20000))


def test_id_and_field_digits():
    ids = [0, 8, 9, 98, 99, 998, 999, 9998, 9999, 99998, 99999, 999998, 999999, 9999998, 9999999, 99999998, 99999999, 999999998,
           999999999, MAX_D - 1]
    assert sorted({len(str(j + 1)) for j in ids}) == list(range(1, 11))
    data = np.arange(1, len(ids) + 1) / 8.0
    indptr = [0, 7, 7, len(ids)]
    check(indptr, ids, data, [1.0, 0.0, -1.0], d=MAX_D)
    check(indptr, ids[::-1], data, [1.0, 0.0, -1.0], fields=ids, d=MAX_D, n_fields=MAX_D)


def test_repeated_and_unsorted_ids_are_written_as_stored():
    ds, want = check([0, 4, 7], [5, 2, 5, 5, 9, 3, 1], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [1.0, 2.0], d=10)
    assert want == b"1.0 6:1.0 3:2.0 6:3.0 6:4.0\n2.0 10:5.0 4:6.0 2:7.0"


@pytest.mark.parametrize("ffm", [False, True])
def test_tokens_straddle_every_boundary(ffm):
    """value lengths cycle 3 .. 24 (22 lengths, coprime to 16 and to 256 items), the ids cycle their digit counts: over 4000
    entries the tokens begin at every offset modulo 16 and every length ends a 256-item span"""
    m = 4000
    data = np.array([value_of_length(3 + q % 22, q) for q in range(m)])
    indices = np.array([10 ** (q % 7) - 1 + (q % 3) for q in range(m)], dtype=np.int64)
    lens = []
    while sum(lens) < m:
        lens.append([5, 0, 17, 1, 40][len(lens) % 5])
    lens[-1] -= sum(lens) - m
    indptr = np.concatenate([[0], np.cumsum(lens)])
    y = np.array([value_of_length(3 + (5 * i) % 22, i) for i in range(len(lens))])
    fields = (np.arange(m) % 11).astype(np.int64) if ffm else None
    ds, want = check(indptr, indices, data, y, fields=fields, d=2000000, chunks=(0, 4096))
    starts = {i % 16 for i, c in enumerate(want) if c == ord(" ")}
    assert starts == set(range(16))


# ---- 5. beyond one pass of every launch --------------------------------------------------------------------------------
def test_beyond_one_pass_of_every_launch():
    """600000 rows of 0 to 3 entries, about 900000 entries: more than n_cu * 8 workgroups of 256 in the length pass (entries and
    rows) and in the write pass (1.5e6 items), so every grid-stride loop goes round"""
    rng = np.random.default_rng(2410)
    n, d = 600000, 50
    lens = rng.integers(0, 4, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    assert n > 524288 and nnz > 524288
    indices = rng.integers(0, d, nnz)
    data = np.round(rng.uniform(-2, 2, nnz), 3)
    y = rng.integers(-1, 2, n).astype(np.float64)
    ds = upload(indptr, indices, data, y, d=d)
    want = oracle_text(indptr.tolist(), indices.tolist(), data.tolist(), y.tolist())
    for chunk in (0, 8 << 20):
        got = nf.formatText(ds, chunkBytes=chunk)
        assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest(), first_difference(got, want)


# ---- 6. y handling and refusals ----------------------------------------------------------------------------------------
def small():
    return upload([0, 2, 3], [0, 3, 1], [0.5, -1.0, 2.0], [0.25, -0.75], d=4)


def test_explicit_and_integer_targets(tmp_path):
    ds = small()
    assert nf.formatText(ds) == b"0.25 1:0.5 4:-1.0\n-0.75 2:2.0"
    assert nf.formatText(ds, y=np.array([3.5, 1e-7])) == b"3.5 1:0.5 4:-1.0\n1e-07 2:2.0"
    assert nf.formatText(ds, y=np.array([1, -1])) == b"1 1:0.5 4:-1.0\n-1 2:2.0"
    assert nf.formatText(ds, y=[0, 9007199254740991]) == b"0 1:0.5 4:-1.0\n9007199254740991 2:2.0"
    assert nf.formatText(ds, y=np.array([1.0, -1.0])) == b"1.0 1:0.5 4:-1.0\n-1.0 2:2.0"
    p = str(tmp_path / "y.txt")
    nf.dumpSVMLightFile(p, ds, np.array([1, -1], dtype=np.int32))
    assert open(p, "rb").read() == b"1 1:0.5 4:-1.0\n-1 2:2.0"
    assert ds.targets().tolist() == [0.25, -0.75]  # the dataset keeps its own


def test_refusals(tmp_path):
    ds = small()
    L = capi.lib()
    n = C.c_int64(0)
    p = str(tmp_path / "x.txt").encode()
    y_bad = np.array([1.0, 0.5])
    for bad in (np.array([1.0, 0.5]), np.array([1.0, 2.0 ** 53]), np.array([np.nan, 1.0]), np.array([np.inf, 1.0])):
        assert L.nfm_dataset_format_text(ds.h, bad.ctypes.data_as(C.c_void_p), 1, 0, None, 0, C.byref(n)) == capi.ERR_INVALID
    assert L.nfm_dataset_dump_svmlight(ds.h, p, y_bad.ctypes.data_as(C.c_void_p), 1, 0) == capi.ERR_INVALID
    assert L.nfm_dataset_format_text(ds.h, None, 1, 0, None, 0, C.byref(n)) == capi.ERR_INVALID  # the dataset's 0.25 with y_int
    with pytest.raises(ValueError, match=r"X\.nSamples != len\(y\)\."):
        nf.formatText(ds, y=[1.0, 2.0, 3.0])
    bare = upload([0, 1], [0], [1.0], d=2)  # no targets
    with pytest.raises(ValueError, match=r"X\.nSamples != len\(y\)\."):
        nf.formatText(bare)
    with pytest.raises(ValueError, match=r"X\.nSamples != len\(y\)\."):
        nf.dumpSVMLightFile(str(tmp_path / "b.txt"), bare)
    assert nf.formatText(bare, y=[2.0]) == b"2.0 1:1.0"
    # the wrong kind
    fa = upload([0, 1], [0], [1.0], [1.0], fields=[0], d=2)
    with pytest.raises(ValueError):
        nf.dumpSVMLightFile(str(tmp_path / "c.txt"), fa)
    with pytest.raises(ValueError):
        nf.dumpFFMFile(str(tmp_path / "c.txt"), ds)
    assert nf.formatText(fa) == b"1.0 1:1:1.0"
    with pytest.raises(ValueError, match="cannot be written"):
        nf.dumpSVMLightFile(str(tmp_path / "no" / "such" / "dir.txt"), ds)
    # length first, then the bytes; a buffer too small
    assert L.nfm_dataset_format_text(ds.h, None, 0, 0, None, 0, C.byref(n)) == capi.NFM_OK
    want = b"0.25 1:0.5 4:-1.0\n-0.75 2:2.0"
    assert n.value == len(want)
    buf = C.create_string_buffer(b"#" * 64, 64)
    m = C.c_int64(0)
    assert L.nfm_dataset_format_text(ds.h, None, 0, 0, buf, 64, C.byref(m)) == capi.NFM_OK
    assert m.value == len(want) and buf.raw[:m.value] == want and buf.raw[m.value:] == b"#" * (64 - m.value)  # no NUL, nothing beyond
    assert L.nfm_dataset_format_text(ds.h, None, 0, 0, buf, len(want) - 1, C.byref(m)) == capi.ERR_INVALID
    assert L.nfm_dataset_format_text(ds.h, None, 0, 16, buf, len(want) - 1, C.byref(m)) == capi.ERR_INVALID  # in pieces too


def test_streamed_dataset_is_refused(tmp_path):
    src = tmp_path / "s.svm"
    src.write_text("1 1:0.5 3:2\n-1 2:1\n")
    fx, fy = str(tmp_path / "s.bin"), str(tmp_path / "s.y")
    nf.convertSVMLightFile(str(src), fx, fy)
    st, _ = nf.newStreamCSRDataset(fx, fy, cacheRows=1)
    assert isinstance(st, nf.StreamCSRDataset)
    for f in (lambda: nf.dumpSVMLightFile(str(tmp_path / "o.txt"), st), lambda: nf.dumpFFMFile(str(tmp_path / "o.txt"), st),
              lambda: nf.formatText(st)):
        with pytest.raises(ValueError, match="resident"):
            f()


# ---- 7. datasets made on the device ------------------------------------------------------------------------------------
def test_datasets_made_on_the_device():
    rng = np.random.default_rng(7)
    indptr, cols, data, y, _ = random_csr(rng, 200, 40, 0.15, False)
    ds = upload(indptr, cols, data, y, d=40)
    rows = rng.integers(0, 200, 150)
    sel = ds[rows]
    sp, si, sd, _ = sel.to_host()
    assert_same_text(nf.formatText(sel, chunkBytes=512), oracle_text(sp, si, sd, y[rows]))
    assert_same_text(nf.formatText(sel), nf.formatText(upload(sp, si, sd, y[rows], d=40)))
    hs = nf.hstack(sel, sel)
    hp, hi, hd, _ = hs.to_host()
    assert hs.nFeatures == 80
    assert_same_text(nf.formatText(hs), nf.formatText(upload(hp, hi, hd, y[rows], d=80)))
    assert_same_text(nf.formatText(hs, chunkBytes=300), oracle_text(hp, hi, hd, y[rows]))
    nf.normalize(hs, axis=1, norm="l2")
    np_, ni, nd, _ = hs.to_host()
    assert not np.array_equal(nd, hd)
    assert_same_text(nf.formatText(hs), nf.formatText(upload(np_, ni, nd, y[rows], d=80)))
    assert_same_text(nf.formatText(hs), oracle_text(np_, ni, nd, y[rows]))


# ---- 8. nfm_format_f64 and the model dump ------------------------------------------------------------------------------
def py_lines(a):
    return "".join(" ".join(host._nim_float(v) for v in r) + "\n" for r in a).encode()


def test_format_f64():
    rng = np.random.default_rng(8)
    vals = special_values()
    for shape in ((1, 1), (3, 7), (1, 1000), (1000, 1), (257, 31)):
        a = rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 12, shape)
        a.ravel()[: min(a.size, len(vals))] = vals[: min(a.size, len(vals))]
        assert_same_text(nf.formatF64(a), py_lines(a))
    a = vals[: len(vals) // 5 * 5].reshape(-1, 5)
    assert_same_text(nf.formatF64(a), py_lines(a))
    L, n = capi.lib(), C.c_int64(0)
    one = np.array([[1.5, -2.0]])
    buf = C.create_string_buffer(4)
    assert L.nfm_format_f64(nf.default_context().h, one.ctypes.data_as(C.c_void_p), 1, 2, buf, 4, C.byref(n)) == capi.ERR_INVALID
    assert L.nfm_format_f64(nf.default_context().h, one.ctypes.data_as(C.c_void_p), 1, 2, None, 0, C.byref(n)) == capi.NFM_OK
    assert n.value == len(b"1.5 -2.0\n")


def model_of(kind, d, k, rng):
    if kind == "fm":
        fm = nf.newFactorizationMachine("regression", degree=2, nComponents=k, warmStart=True)
        fm.set_params(rng.standard_normal((1, k, d)) * 10.0 ** rng.integers(-9, 9, (1, k, d)), rng.standard_normal(d), 0.125)
    elif kind == "ffm":
        fm = nf.newFieldAwareFactorizationMachine("classification", nComponents=k, warmStart=True)
        fm.set_params(rng.standard_normal((2, d, k)) * 10.0 ** rng.integers(-9, 9, (2, d, k)), rng.standard_normal(d), -3.5)
    else:
        fm = nf.newConvexFactorizationMachine("regression", maxComponents=k + 2)
        fm.set_params(rng.standard_normal((k, d)) * 10.0 ** rng.integers(-9, 9, (k, d)), rng.standard_normal(k), rng.standard_normal(d), 1e-30)
    return fm


@pytest.mark.parametrize("kind", ["fm", "ffm", "cfm"])
@pytest.mark.parametrize("shape", [(4096, 16), (7, 3)], ids=["4096x16", "7x3"])
def test_model_dump_keeps_its_bytes(kind, shape, tmp_path, monkeypatch):
    d, k = shape
    fm = model_of(kind, d, k, np.random.default_rng(9))
    calls = []
    real = host.formatF64
    monkeypatch.setattr(host, "formatF64", lambda a, ctx=None: (calls.append(np.shape(a)), real(a, ctx))[1])
    on_device = str(tmp_path / "device.txt")
    fm.dump(on_device)
    assert (len(calls) > 0) == (d * k >= 65536), calls  # the large block went through nfm_format_f64, the small model did not
    n_calls = len(calls)
    monkeypatch.setattr(host, "_DUMP_DEVICE_MIN", 1 << 62)  # the Python lines alone
    in_python = str(tmp_path / "python.txt")
    fm.dump(in_python)
    assert len(calls) == n_calls
    with open(on_device, "rb") as f, open(in_python, "rb") as g:
        assert_same_text(f.read(), g.read())
    back = nf.load(on_device, False)
    assert type(back) is type(fm)
    assert np.array_equal(np.asarray(back.P).view(np.uint64), np.asarray(fm.P).view(np.uint64))
    assert np.array_equal(np.asarray(back.w).view(np.uint64), np.asarray(fm.w).view(np.uint64))
    assert back.intercept == fm.intercept
    if kind == "cfm":
        assert np.array_equal(np.asarray(back.lams), np.asarray(fm.lams))
