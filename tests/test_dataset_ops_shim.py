"""The Nim side of the dataset ops (nim/hip_dataset.nim and its declarations in nim/nimfm_hip.nim) cannot be compiled here, so
it is held to include/nimfm_hip.h mechanically, as tests/test_psgd_shim.py holds PSGD's file.  No GPU."""
import inspect
import os
import re

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = ("nfm_dataset_select_rows", "nfm_dataset_slice_rows", "nfm_dataset_vstack", "nfm_dataset_hstack", "nfm_dataset_normalize",
           "nfm_dataset_load_user_item", "nfm_dataset_parse_user_item", "nfm_rng_shuffle_forward")


def test_declarations_match_the_header():
    hdr, h = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    assert hdr["nfm_dataset_vstack"][1] == ["ptr NfmDataset", "int64", "ptr NfmDataset"]  # an array of handles, then the result
    assert hdr["nfm_dataset_normalize"][1] == ["NfmDataset", "int32", "int32", "ptr NfmDataset"]
    # NormKind in the reference's order (tensor/sparse.nim:37-38: l1, l2, linfty): ord(norm) crosses the boundary
    assert re.search(r"NFM_NORM_L1 = 0, NFM_NORM_L2 = 1, NFM_NORM_LINFTY = 2", h)


def test_the_include_file_calls_only_declared_entry_points():
    nim, core = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_dataset.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRIES) - {"nfm_dataset_parse_user_item", "nfm_rng_shuffle_forward"} <= calls
    for call in calls:
        assert call in nim, "hip_dataset.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    # the reference's names and signatures on the device dataset type
    for sig in (r"proc `\[\]`\*\(X: ref HipDatasetObj, indicesRow: openarray\[int\]\)",
                r"proc `\[\]`\*\(X: ref HipDatasetObj, slice: Slice\[int\]\)",
                r"proc `\[\]`\*\(X: ref HipDatasetObj, slice: HSlice\[int, BackwardsIndex\]\)",
                r"proc shuffle\*\[U\]\(X: ref HipDatasetObj, y: seq\[U\], indices: openarray\[int\]\)",
                r"proc shuffle\*\[U\]\(X: ref HipDatasetObj, y: seq\[U\]\)",
                r"proc vstack\*\(dataseq: varargs\[ref HipDatasetObj\]\)", r"proc hstack\*\(dataseq: varargs\[ref HipDatasetObj\]\)",
                r"proc normalize\*\(X: ref HipDatasetObj, axis = 1, norm: NormKind = l2\)",
                r"proc loadUserItemRatingFile\*\(f: string, X: var HipCSRDataset, y: var seq\[float64\]\)"):
        assert re.search(sig, flat), sig
    # X[a..b] is inclusive in Nim, the entry's range is half open; a..^b as dataset.nim:335
    assert "slice.a.int64, (slice.b + 1).int64" in flat and "X[slice.a..(X.nSamples - int(slice.b))]" in flat
    # the forward draw, dataset.nim:388-394, from Nim's own generator
    assert "j = rand(len(y)-1-i)" in flat and "indices[i] = indices[i+j]" in flat and "indices[i+j] = tmp" in flat
    assert flat.count('raise newException(ValueError, "X.nSamples != len(y)")') == 2
    # normalize swaps the handle and frees the old arrays
    assert flat.index("nfm_dataset_normalize(") < flat.index("nfm_dataset_destroy(X.handle)") < flat.index("X.handle = h")
    assert "ord(norm).int32" in flat
    assert "when defined(nimfmHip): include hip_dataset" in core
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hip_dataset.nim" in integ and "when defined(nimfmHip): include hip_dataset" in integ


def test_the_three_hosts_agree_on_names_and_defaults():
    import nimfm_amd as nf
    for name in ("shuffle", "vstack", "hstack", "normalize", "loadUserItemRatingFile"):
        assert callable(getattr(nf, name)), name
    sig = inspect.signature(nf.normalize)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("axis", 1), ("norm", "l2")]
    assert list(inspect.signature(nf.shuffle).parameters) == ["X", "y", "indices"]
    assert hasattr(nf.CSRDataset, "__getitem__")
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("enum NormKind { l1 = 0, l2 = 1, linfty = 2 };", "inline void normalize(CSRDataset& X, int axis = 1, NormKind norm = l2)",
                  "inline CSRDataset vstack(", "inline CSRDataset hstack(", "CSRDataset operator[](const std::vector<int64_t>& indicesRow) const",
                  "CSRDataset slice(int64_t begin, int64_t end) const", "inline void loadUserItemRatingFile(const std::string& f, CSRDataset& X, std::vector<double>& y",
                  "shuffle(const CSRDataset& X, const std::vector<U>& y, const std::vector<int64_t>& indices)", "nfm_rng_shuffle_forward("):
        assert piece in hpp, piece


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table
    assert _capi.NORM == {"l1": 0, "l2": 1, "linfty": 2}


def test_hosts_refuse_what_is_not_a_resident_dataset_before_any_device_call():
    import pytest

    import nimfm_amd as nf

    class NotResident:  # stands for a StreamCSRDataset: anything that is not a CSRDataset
        nSamples = 3

    for call in (lambda: nf.shuffle(NotResident(), [0.0] * 3), lambda: nf.vstack(NotResident()), lambda: nf.hstack(NotResident(), NotResident()),
                 lambda: nf.normalize(NotResident())):
        with pytest.raises(ValueError, match="resident on the device"):
            call()
    assert not hasattr(nf.StreamCSRDataset, "__getitem__")
