"""The column-major dataset across the three hosts: the new entry points of include/nimfm_hip.h against nimfm_amd/_capi.py and
nim/nimfm_hip.nim, the Python signatures and defaults, the Nim overload names (nim/hip_dataset.nim and the CD-family files
cannot be compiled here, so they are held to the header mechanically, as tests/test_dataset_ops_shim.py does).  No GPU."""
import inspect
import os
import re

import pytest

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = ("nfm_dataset_create_csc", "nfm_dataset_create_csc_device", "nfm_dataset_to_csc", "nfm_dataset_to_csr", "nfm_dataset_layout",
           "nfm_dataset_get_csc", "nfm_dataset_load_user_item_lines", "nfm_dataset_parse_user_item_lines")


def test_declarations_match_the_header():
    hdr, h = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    assert hdr["nfm_dataset_to_csc"][1] == hdr["nfm_dataset_to_csr"][1] == ["NfmDataset", "ptr NfmDataset"]
    assert hdr["nfm_dataset_layout"][1] == ["NfmDataset", "ptr int32"]
    assert hdr["nfm_dataset_get_csc"][1] == ["NfmDataset", "ptr int64", "ptr int64", "ptr float64"]
    # the switch is a new entry: the prototypes of the existing loaders are what they were
    assert hdr["nfm_dataset_load_user_item"][1] == ["NfmCtx", "cstring", "ptr NfmDataset"]
    assert hdr["nfm_dataset_parse_user_item"][1] == ["NfmCtx", "cstring", "int64", "ptr NfmDataset"]
    assert hdr["nfm_dataset_load_user_item_lines"][1] == ["NfmCtx", "cstring", "int32", "ptr NfmDataset"]
    assert re.search(r"NFM_LAYOUT_CSR = 0, NFM_LAYOUT_CSC = 1", h)
    # every entry cites the reference proc it replaces
    raw = open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    for cite in ("dataset.nim:124-129", "tensor/sparse.nim:510-527", ":490-507", "tensor/sparse.nim:300-330", ":583-610", ":701-716", ":414-427",
                 "dataset.nim:923, 955, 975", "dataset.nim:903-992"):
        assert cite in raw, cite


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table
    assert _capi.LAYOUT == {"csr": 0, "csc": 1}


def test_python_names_signatures_and_defaults():
    import nimfm_amd as nf
    for name in ("CSCDataset", "newCSCDataset", "toCSCDataset", "toCSRDataset"):
        assert hasattr(nf, name), name
    assert list(inspect.signature(nf.newCSCDataset).parameters) == ["data", "indices", "indptr", "nSamples", "nFeatures", "ctx"]
    assert list(inspect.signature(nf.newCSCDataset).parameters)[:5] == list(inspect.signature(nf.newCSRDataset).parameters)[:5]
    for fn in (nf.loadSVMLightFile, nf.loadUserItemRatingFile, nf.parseUserItemRatingText, nf.parseText):
        assert inspect.signature(fn).parameters["layout"].default == "csr", fn.__name__
    for attr in ("from_device", "to_host", "targets", "set_targets", "nFeatures", "shape", "__getitem__"):
        assert hasattr(nf.CSCDataset, attr), attr
    assert issubclass(nf.CSCDataset, nf.CSRDataset)  # what takes a resident dataset takes either; the layout decides
    # the column-wise solvers accept a CSCDataset, every other solver refuses it before any device call
    assert nf.CD._col_wise and nf.PCD._col_wise and nf.PBCD._col_wise
    assert not nf.PGD._col_wise and not nf.FISTA._col_wise and not nf.NMAPGD._col_wise and not nf.Katyusha._col_wise


def test_hosts_refuse_before_any_device_call():
    import nimfm_amd as nf
    from nimfm_amd import host

    X = nf.CSCDataset.__new__(nf.CSCDataset)  # no handle: nothing below may reach the library
    X.h, X.nSamples, X._nFeatures, X.nFields, X.nnz, X.ctx, X._keep = None, 3, 2, 0, 0, None, None
    with pytest.raises(ValueError, match="toCSRDataset"):
        host._row_major(X, "newSGD")
    with pytest.raises(ValueError, match="not supported for CSCMatrix"):
        X[[0, 1]]
    with pytest.raises(ValueError, match="toCSRDataset"):
        nf.shuffle(X, [0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="toCSRDataset"):
        nf.formatText(X)
    with pytest.raises(ValueError, match="toCSRDataset"):
        nf.newSGD(verbose=0).fit(X, [0.0] * 3, nf.newFactorizationMachine("regression"))
    with pytest.raises(ValueError, match="layout"):
        nf.parseUserItemRatingText("1 1 5\n", ctx=object(), layout="coo")
    with pytest.raises(ValueError, match="field-aware"):
        nf.CSCDataset([1.0], [0], [0, 1], 1, 1, fields=[0], nFields=1, ctx=object())
    with pytest.raises(ValueError, match=r"len\(indptr\) != nFeatures \+ 1"):
        nf.CSCDataset([1.0], [0], [0, 1], 1, 2, ctx=object())


def test_nim_overloads():
    nim, core = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_dataset.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_dataset_create_csc", "nfm_dataset_to_csc", "nfm_dataset_to_csr", "nfm_dataset_load_user_item_lines"} <= calls
    for call in calls:
        assert call in nim, "hip_dataset.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    for sig in (r"HipCSCDataset\* = distinct HipCSRDataset",
                r"proc toHip\*\(X: CSCDataset\): HipCSCDataset",
                r"proc toCSCDataset\*\(X: HipCSRDataset\): HipCSCDataset",
                r"proc toCSRDataset\*\(X: HipCSCDataset\): HipCSRDataset",
                r"proc loadSVMLightFile\*\(f: string, dataset: var HipCSCDataset, y: var seq\[float64\], nFeatures: int = -1\)",
                r"proc loadUserItemRatingFile\*\(f: string, X: var HipCSCDataset, y: var seq\[float64\]\)",
                r"proc `\[\]`\*\(X: HipCSCDataset, slice: Slice\[int\]\): HipCSCDataset",
                r"proc `\[\]`\*\(X: HipCSCDataset, slice: HSlice\[int, BackwardsIndex\]\): HipCSCDataset",
                r"proc vstack\*\(dataseq: varargs\[HipCSCDataset\]\): HipCSCDataset",
                r"proc hstack\*\(dataseq: varargs\[HipCSCDataset\]\): HipCSCDataset",
                r"proc normalize\*\(X: HipCSCDataset, axis = 1, norm: NormKind = l2\)",
                r"proc decisionFunction\*\(self: FactorizationMachine, X: HipCSCDataset\): seq\[float64\]"):
        assert re.search(sig, flat), sig
    # no X[indices] and no shuffle for the column type: the reference has none (tensor/sparse.nim:298)
    assert not re.search(r"proc `\[\]`\*\(X: HipCSCDataset, indicesRow", flat) and not re.search(r"proc shuffle\*[^)]*HipCSCDataset", flat)
    # the rating loader of the column type skips lines of fewer than 5 characters
    assert "nfm_dataset_load_user_item_lines(hipContext(), f.cstring, 1'i32, addr h)" in flat
    # the column solvers take the reference's own dataset type and run on the row twin
    for fname, head in (("hip_cd.nim", r"proc fit\*\[L\]\(self: CD\[L\], X: HipCSCDataset,"),
                        ("hip_pcd.nim", r"proc fit\*\[L, R\]\(self: PCD\[L, R\], X: HipCSCDataset,"),
                        ("hip_pbcd.nim", r"proc fit\*\[L, R\]\(self: PBCD\[L, R\], X: HipCSCDataset,"),
                        ("hip_hazan.nim", r"proc fit\*\(self: Hazan, X: HipCSCDataset,"),
                        ("hip_gcd.nim", r"proc fit\*\[L\]\(self: GreedyCD\[L\], X: HipCSCDataset,")):
        text = " ".join(re.sub(r"##.*", "", open(os.path.join(NIM, fname)).read()).split())
        assert re.search(head, text), fname
        assert "fit(self, rowsOf(X), y," in text, fname
    assert re.search(r"proc decisionFunction\*\(self: ConvexFactorizationMachine, X: HipCSCDataset\)", open(os.path.join(NIM, "hip_hazan.nim")).read())
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "HipCSCDataset" in integ


def test_cpp_host_names():
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("class CSCDataset : public CSRDataset", "inline CSCDataset toCSCDataset(const CSRDataset& X)",
                  "inline CSRDataset toCSRDataset(const CSRDataset& X)", "CSCDataset slice(int64_t begin, int64_t end) const",
                  "inline CSCDataset vstack(std::initializer_list<const CSCDataset*> dataseq)",
                  "inline CSCDataset hstack(std::initializer_list<const CSCDataset*> dataseq)", "nfm_dataset_create_csc(", "nfm_dataset_get_csc(",
                  "nfm_dataset_load_user_item_lines(default_context(), f.c_str(), 1, &hr)"):
        assert piece in hpp, piece
