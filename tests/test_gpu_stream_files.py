"""The binary stream files on the device: formatStream / dumpStreamFile, newStreamCSCDataset,
transposeFile and convertFFMFile against the plain restatements of tests/stream_file_restatement.py.  Every byte comparison is
exact and against the restatement, never against the code under test.  All shapes are tiny."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import nimfm_amd as nf
import stream_file_restatement as R
from nimfm_amd import _capi as capi
from oracle import ingest

pytestmark = pytest.mark.gpu
I64 = np.int64


def pieces_of_last_call():
    p, b = C.c_int64(), C.c_int64()
    capi.check(capi.lib().nfm_dump_stats(C.byref(p), C.byref(b), None, None, None))
    return p.value, b.value


def transpose_arrays(indptr, indices, data, n_out):
    """the arrays of the other orientation, as transpose_plain orders them"""
    cols = [[] for _ in range(n_out)]
    for r in range(len(indptr) - 1):
        for q in range(indptr[r], indptr[r + 1]):
            cols[indices[q]].append((data[q], r))
    ip = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(I64)
    idx = np.array([r for c in cols for _, r in c], dtype=I64)
    val = np.array([v for c in cols for v, _ in c], dtype=np.float64)
    return ip, idx, val


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (kind, indptr, indices, data, fields, nSamples, nFeatures, nFields): made once, never modified"""
    rng = np.random.default_rng(26)
    out = {"one": ("csr", np.array([0, 1], dtype=I64), np.array([0], dtype=I64), np.array([2.5]), None, 1, 1, 0)}
    ip, idx, val = R.matrix_37x11(rng)
    out["m37x11"] = ("csr", ip, idx, val, None, 37, 11, 0)
    out["m37x11_csc"] = ("csc",) + transpose_arrays(ip, idx, val, 11) + (None, 37, 11, 0)
    ipf, idxf, valf = R.random_records(rng, 23, 17, 0.4, empty=(3, 22))
    out["field9"] = ("csrfield", ipf, idxf, valf, rng.integers(0, 9, len(valf)).astype(I64), 23, 17, 9)
    out["all_empty"] = ("csr", np.zeros(8, dtype=I64), np.zeros(0, dtype=I64), np.zeros(0), None, 7, 5, 0)
    ipl, idxl, vall = R.long_record(rng)
    out["long"] = ("csr", ipl, idxl, vall, None, len(ipl) - 1, 6000, 0)
    # field-aware over several tiles of 2048 words: 24-byte elements straddle tile boundaries and 16-byte vectors at every phase
    ipb, idxb, valb = R.random_records(rng, 300, 40, 0.35, empty=(0, 7, 299))
    out["field_tiles"] = ("csrfield", ipb, idxb, valb, rng.integers(0, 9, len(valb)).astype(I64), 300, 40, 9)
    # thousands of empty and one-entry records: far more than 256 record starts inside one tile
    ips, idxs, vals = R.random_records(rng, 5000, 7, 0.07, first_id_present=False)
    out["many_short"] = ("csr", ips, idxs, vals, None, 5000, 7, 0)
    out["many_short_field"] = ("csrfield", ips, idxs, vals, rng.integers(0, 3, len(vals)).astype(I64), 5000, 7, 3)
    for v in out.values():
        for a in v[1:5]:
            if a is not None:
                a.setflags(write=False)
    return out


def dataset(name):
    kind, ip, idx, val, fld, n, d, nf_ = shapes()[name]
    if kind == "csc":
        return nf.newCSCDataset(val, idx, ip, n, d)
    if kind == "csrfield":
        return nf.newCSRFieldDataset(val, idx, ip, fld, n, d, nf_)
    return nf.newCSRDataset(val, idx, ip, n, d)


def want_bytes(name):
    kind, ip, idx, val, fld, n, d, nf_ = shapes()[name]
    return R.write_stream(ip, idx, val, fld, kind, n, d, nf_)


def mid_record_bytes(name):
    kind, ip = shapes()[name][:2]
    sizes = sorted(8 + (24 if kind == "csrfield" else 16) * int(c) for c in np.diff(ip))
    return sizes[len(sizes) // 2]


# ---- 1. formatStream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "m37x11", "m37x11_csc", "field9", "all_empty", "long", "field_tiles", "many_short", "many_short_field"])
def test_format_stream_bytes(name):
    X = dataset(name)
    want = want_bytes(name)
    fielded = shapes()[name][0] == "csrfield"
    assert len(want) == (62 if fielded else 49) + 8 * (len(shapes()[name][1]) - 1) + (24 if fielded else 16) * len(shapes()[name][3])
    if name == "field_tiles":
        assert len(want) > 6 * 2048 * 8  # several tiles
    if name.startswith("many_short"):
        ip = shapes()[name][1]
        assert np.diff(ip).max() <= 4 and (len(want) - 49) // 8 // 2048 >= 2 and (np.diff(ip) == 0).sum() > 2000
    n_records = len(shapes()[name][1]) - 1
    for chunk in (0, 24, mid_record_bytes(name), 4096):
        got = nf.formatStream(X, chunkBytes=chunk)
        assert got == want, (name, chunk, len(got), len(want))
        p, b = pieces_of_last_call()
        assert b == len(want)
        if chunk == 24 and n_records > 1:
            assert p > 1, (name, p)  # at most a count word and ... nothing more: every record with an entry is cut off
        if chunk == 0:
            assert p == 1
    if name == "long":  # the long record is a piece by itself at 4096 and spans many tiles
        nf.formatStream(X, chunkBytes=4096)
        assert pieces_of_last_call()[0] == 3
    if name == "m37x11":  # toCSCDataset's columns are the restatement's
        assert nf.formatStream(nf.toCSCDataset(X)) == want_bytes("m37x11_csc")


def test_format_stream_buffer_conventions():
    X = dataset("m37x11")
    want = want_bytes("m37x11")
    n = C.c_int64(0)
    capi.check(capi.lib().nfm_dataset_format_stream(X.h, 0, None, 0, C.byref(n)))
    assert n.value == len(want)
    buf = C.create_string_buffer(len(want) - 1)
    assert capi.lib().nfm_dataset_format_stream(X.h, 0, buf, len(want) - 1, C.byref(n)) == capi.ERR_INVALID
    assert n.value == len(want)


@pytest.mark.parametrize("vals,vmax,vmin", [([0.0, -0.0, 1.0], 1.0, 0.0), ([-0.0, 0.0], -0.0, -0.0),
                                            ([float("nan"), 2.0, float("nan"), -3.0], 2.0, -3.0), ([float("nan")], float("-inf"), float("inf"))])
def test_header_max_min_are_the_ordered_fold(vals, vmax, vmin):
    m = len(vals)
    X = nf.newCSRDataset(np.array(vals), np.arange(m, dtype=I64), np.array([0, m], dtype=I64), 1, m)
    got = nf.formatStream(X)
    assert got == R.write_stream([0, m], list(range(m)), vals, None, "csr", 1, m)
    assert got[33:41] == struct.pack("<d", vmax) and got[41:49] == struct.pack("<d", vmin)


# ---- 2. round trips ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m37x11", "field9", "long"])
def test_dump_reloads_row_major(name, tmp_path):
    kind, ip, idx, val, fld, n, d, nf_ = shapes()[name]
    y = np.arange(n, dtype=np.float64) - 3.5
    (tmp_path / "y.bin").write_bytes(y.tobytes())
    nf.dumpStreamFile(str(tmp_path / "x.bin"), dataset(name), chunkBytes=4096)
    assert (tmp_path / "x.bin").read_bytes() == want_bytes(name)
    ds, y2 = nf.newStreamCSRDataset(str(tmp_path / "x.bin"), str(tmp_path / "y.bin"))
    ip2, idx2, val2, fld2 = ds.to_host()
    assert (ds.nSamples, ds.nFeatures, ds.nFields) == (n, d, nf_)
    assert ip2.tobytes() == ip.tobytes() and idx2.tobytes() == idx.tobytes() and val2.tobytes() == val.tobytes()
    assert (fld2 is None) if fld is None else fld2.tobytes() == fld.tobytes()
    assert y2.tobytes() == y.tobytes() and nf.loadStreamLabel(str(tmp_path / "y.bin")).tobytes() == y.tobytes()


def test_dump_reloads_column_major(tmp_path):
    kind, ip, idx, val, _, n, d, _ = shapes()["m37x11_csc"]
    y = np.linspace(-1, 1, n)
    (tmp_path / "y.bin").write_bytes(y.tobytes())
    nf.dumpStreamFile(str(tmp_path / "c.bin"), dataset("m37x11_csc"))
    assert (tmp_path / "c.bin").read_bytes() == want_bytes("m37x11_csc")
    ds, y2 = nf.newStreamCSCDataset(str(tmp_path / "c.bin"), str(tmp_path / "y.bin"))
    assert isinstance(ds, nf.CSCDataset) and (ds.nSamples, ds.nFeatures) == (n, d)
    ip2, idx2, val2 = ds.to_host()
    assert ip2.tobytes() == ip.tobytes() and idx2.tobytes() == idx.tobytes() and val2.tobytes() == val.tobytes()
    assert y2.tobytes() == y.tobytes()
    ds0, y0 = nf.newStreamCSCDataset(str(tmp_path / "c.bin"))
    assert np.array_equal(y0, np.zeros(n))


# ---- 3. transposeFile ----------------------------------------------------------------------------------------------------------
def transposable(name):
    """the matrix as a STREAMCSR file whose header carries max / min unrelated to the data"""
    kind, ip, idx, val, _, n, d, _ = shapes()[name]
    return R.write_stream(ip, idx, val, None, "csr", n, d, vmax=123.0, vmin=-7.0)


@pytest.mark.parametrize("name", ["m37x11", "long"])
def test_transpose_file_both_directions(name, tmp_path):
    x = transposable(name)
    nnz = len(shapes()[name][3])
    a, b, c, e = (str(tmp_path / f) for f in ("a.bin", "b.bin", "c.bin", "e.bin"))
    (tmp_path / "a.bin").write_bytes(x)
    want_c = R.transpose_literal(x, nnz)
    assert want_c == R.transpose_plain(x) and want_c[9:49] == x[9:49]
    nf.transposeFile(a, b)
    got = (tmp_path / "b.bin").read_bytes()
    assert got == want_c
    assert struct.unpack_from("<dd", got, 33) == (123.0, -7.0)
    nf.transposeFile(a, e, cacheSize=1, chunkBytes=4096)
    assert (tmp_path / "e.bin").read_bytes() == want_c
    if shapes()[name][1][1] > 0:  # back: the first row has entries
        nf.transposeFile(b, c)
        assert (tmp_path / "c.bin").read_bytes() == R.transpose_literal(want_c, nnz)
    else:  # the 37 x 11 matrix has an empty first row: the reference does not terminate on its CSC file
        with pytest.raises(R.DoesNotTerminate):
            R.transpose_literal(want_c, nnz, max_passes=20)
        with pytest.raises(ValueError, match="does not terminate"):
            nf.transposeFile(b, c)
        # without that row, both ways
        kind, ip, idx, val, _, n, d, _ = shapes()[name]
        x1 = R.write_stream(ip[1:], idx, val, None, "csr", n - 1, d, vmax=123.0, vmin=-7.0)
        (tmp_path / "a1.bin").write_bytes(x1)
        nf.transposeFile(str(tmp_path / "a1.bin"), b)
        c1 = (tmp_path / "b.bin").read_bytes()
        assert c1 == R.transpose_literal(x1, nnz)
        nf.transposeFile(b, c)
        assert (tmp_path / "c.bin").read_bytes() == R.transpose_literal(c1, nnz)


def test_transpose_file_refusals(tmp_path):
    out = str(tmp_path / "out.bin")

    def put(name, data):
        (tmp_path / name).write_bytes(data)
        return str(tmp_path / name)

    rng = np.random.default_rng(3)
    ip, idx, val = R.random_records(rng, 6, 5, 0.6)
    idx = np.where(idx == 0, 1, idx)  # no id 0: the first output record would be empty
    with pytest.raises(ValueError, match="first record of the transposed file would be empty.*does not terminate"):
        nf.transposeFile(put("e.bin", R.write_stream(ip, idx, val, None, "csr", 6, 5)), out)
    with pytest.raises(ValueError, match="does not terminate"):
        nf.transposeFile(put("z.bin", R.write_stream(np.zeros(4, dtype=I64), [], [], None, "csr", 3, 2)), out)
    _, ipf, idxf, valf, fld, n, d, nf_ = shapes()["field9"]
    with pytest.raises(nf.NfmError, match="FIELD") as ei:
        nf.transposeFile(put("f.bin", R.write_stream(ipf, idxf, valf, fld, "csrfield", n, d, nf_)), out)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="not neither StreamCSC nor StreamCSR"):
        nf.transposeFile(put("j.bin", b"hello world, not a matrix at all, but long enough to hold a header"), out)
    good = transposable("m37x11")
    with pytest.raises(ValueError, match="overruns|truncated|entries"):
        nf.transposeFile(put("t.bin", good[:-5]), out)
    n_, d_, nnz_ = struct.unpack_from("<qqq", good, 9)
    with pytest.raises(ValueError, match="outside"):
        nf.transposeFile(put("c.bin", good[:9] + struct.pack("<qqq", n_, d_ // 2, nnz_) + good[33:]), out)
    csc = R.transpose_plain(good)
    with pytest.raises(ValueError, match=r"outside \[0, nRows\)"):
        nf.transposeFile(put("r.bin", csc[:9] + struct.pack("<qqq", n_ // 2, d_, nnz_) + csc[33:]), out)
    assert not (tmp_path / "out.bin").exists()  # nothing was written for a refused file


# ---- 4. newStreamCSCDataset ------------------------------------------------------------------------------------------------
def test_stream_csc_dataset_columns_and_cd(tmp_path):
    rng = np.random.default_rng(40)
    n, d = 40, 12
    ip, idx, val = R.random_records(rng, n, d, 0.3)
    y = rng.standard_normal(n)
    x = R.write_stream(ip, idx, val, None, "csr", n, d)
    c = R.transpose_plain(x)
    (tmp_path / "r.bin").write_bytes(x)
    (tmp_path / "c.bin").write_bytes(c)
    (tmp_path / "y.bin").write_bytes(y.tobytes())
    dc, yc = nf.newStreamCSCDataset(str(tmp_path / "c.bin"), str(tmp_path / "y.bin"))
    _, _, cip, cidx, cval = R.read_plain(c)
    got = dc.to_host()
    assert got[0].tobytes() == cip.tobytes() and got[1].tobytes() == cidx.tobytes() and got[2].tobytes() == cval.tobytes()
    assert yc.tobytes() == y.tobytes()
    dr, yr = nf.newStreamCSRDataset(str(tmp_path / "r.bin"), str(tmp_path / "y.bin"))
    fits = []
    for X in (dc, nf.toCSCDataset(dr)):
        fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3)
        nf.randomize(1)
        nf.newCD(maxIter=2, tol=0, verbose=0).fit(X, y, fm)
        fits.append((np.asarray(fm.w).tobytes(), np.asarray(fm.P).tobytes(), struct.pack("<d", fm.intercept)))
    assert fits[0] == fits[1]
    assert np.isfinite(np.frombuffer(fits[0][1])).all() and np.any(np.frombuffer(fits[0][1]) != 0)
    # each loader refuses the other's file and names the one that reads it
    with pytest.raises(nf.NfmError, match="nfm_dataset_load_stream") as ei:
        nf.newStreamCSCDataset(str(tmp_path / "r.bin"))
    assert ei.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(nf.NfmError, match=r"column-major \(STREAMCSC\) file; the row-wise optimizers need STREAMCSR") as ei:
        nf.newStreamCSRDataset(str(tmp_path / "c.bin"))
    assert ei.value.code == capi.ERR_UNSUPPORTED
    # validation mirrors the row-major loader's
    (tmp_path / "t.bin").write_bytes(c[:-5])
    with pytest.raises(ValueError, match="overruns|truncated"):
        nf.newStreamCSCDataset(str(tmp_path / "t.bin"))
    (tmp_path / "p.bin").write_bytes(c[:9] + struct.pack("<qqq", n, 1 << 30, len(val)) + c[33:])
    with pytest.raises(ValueError, match="promises"):
        nf.newStreamCSCDataset(str(tmp_path / "p.bin"))
    (tmp_path / "s.bin").write_bytes(c[:9] + struct.pack("<qqq", n, d, len(val) + 1) + c[33:])
    with pytest.raises(ValueError, match="header says"):
        nf.newStreamCSCDataset(str(tmp_path / "s.bin"))
    (tmp_path / "y3.bin").write_bytes(y[:-1].tobytes())
    with pytest.raises(ValueError, match="labels"):
        nf.newStreamCSCDataset(str(tmp_path / "c.bin"), str(tmp_path / "y3.bin"))
    with pytest.raises(ValueError, match="not a StreamCSC"):
        (tmp_path / "j.bin").write_bytes(b"hello world, not a matrix")
        nf.newStreamCSCDataset(str(tmp_path / "j.bin"))


# ---- 5. convertFFMFile -----------------------------------------------------------------------------------------------------
def ffm_text(base_field, base_index, rng):
    rows = []
    for i in range(19):
        m = int(rng.integers(0, 6)) if i != 4 else 0
        ent = ["%d:%d:%s" % (int(rng.integers(0, 5)) + base_field, int(rng.integers(0, 30)) + base_index, repr(float(np.round(rng.standard_normal(), 4))))
               for _ in range(m)]
        rows.append(" ".join([repr(float(i % 3) - 1.0)] + ent))
    rows[0] = "1.0 %d:%d:0.25 %d:%d:-1.5" % (base_field, base_index, base_field + 4, base_index + 29)  # the whole ranges occur
    return "\n".join(rows) + "\n"


@pytest.mark.parametrize("base_field,base_index", [(0, 0), (1, 1), (1, 3)])
def test_convert_ffm_file(base_field, base_index, tmp_path):
    text = ffm_text(base_field, base_index, np.random.default_rng(50 + base_index))
    (tmp_path / "in.ffm").write_text(text)
    xb, yb = R.convert_ffm(text)
    x, y = str(tmp_path / "x.bin"), str(tmp_path / "y.bin")
    nf.convertFFMFile(str(tmp_path / "in.ffm"), x, y)
    assert (tmp_path / "x.bin").read_bytes() == xb and (tmp_path / "y.bin").read_bytes() == yb
    if base_field == 0:  # 0-based fields stay below nFields: the file reloads to what loadFFMFile gives
        ds, y2 = nf.newStreamCSRDataset(x, y)
        ref, yref = nf.loadFFMFile(str(tmp_path / "in.ffm"))
        for a, b in zip(ds.to_host(), ref.to_host()):
            assert a.tobytes() == b.tobytes()
        assert (ds.nSamples, ds.nFeatures, ds.nFields) == (ref.nSamples, ref.nFeatures, ref.nFields) and y2.tobytes() == yref.tobytes()
    else:  # a field equal to nFields was written (the reference shifts the ids only): the loader goes on refusing it
        with pytest.raises(ValueError, match=r"field outside \[0, nFields\)"):
            nf.newStreamCSRDataset(x, y)


def test_convert_ffm_errors(tmp_path):
    x, y = str(tmp_path / "x.bin"), str(tmp_path / "y.bin")
    (tmp_path / "a.ffm").write_text("1 -1:-2:0.5\n")
    with pytest.raises(ValueError, match="Negative field index is included."):
        nf.convertFFMFile(str(tmp_path / "a.ffm"), x, y)
    (tmp_path / "b.ffm").write_text("1 0:-2:0.5\n")
    with pytest.raises(ValueError, match="Negative index is included."):
        nf.convertFFMFile(str(tmp_path / "b.ffm"), x, y)


def test_convert_svmlight_goes_through_the_packer(tmp_path):
    """bytes as before (tests/test_gpu_ingest.py::test_stream_files holds them too), and the pack kernel ran"""
    text = "1 3:0.5 7:-0.0 4:0.0\n-1 5:2\n0.5 3:1e-3\n"
    (tmp_path / "in.svm").write_text(text)
    ctx = nf.default_context()
    L = capi.lib()
    capi.check(L.nfm_ctx_timing_enable(ctx.h, 1))
    try:
        capi.check(L.nfm_ctx_timing_reset(ctx.h))
        nf.convertSVMLightFile(str(tmp_path / "in.svm"), str(tmp_path / "x.bin"), str(tmp_path / "y.bin"))
        n, ms = C.c_int64(), C.c_double()
        capi.check(L.nfm_ctx_timing_get(ctx.h, b"stream_pack", C.byref(n), C.byref(ms)))
        assert n.value == 1
    finally:
        capi.check(L.nfm_ctx_timing_enable(ctx.h, 0))
    xb, yb = ingest.convert_svmlight(text)
    assert (tmp_path / "x.bin").read_bytes() == xb and (tmp_path / "y.bin").read_bytes() == yb
    assert xb[41:49] == struct.pack("<d", -0.0)  # min: -0.0 comes before 0.0 in the file
