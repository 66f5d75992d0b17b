"""The binary stream files across the three hosts: the five entry points of include/nimfm_hip.h against
nimfm_amd/_capi.py, nim/nimfm_hip.nim and nimfm_amd/host/nimfm.hpp, and the host names with the reference's parameter names
(nim/hip_dataset.nim cannot be compiled here, so it is held to the header mechanically, as tests/test_csc_shim.py does).  No GPU."""
import inspect
import os
import re

import pytest

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = ("nfm_dataset_dump_stream", "nfm_dataset_format_stream", "nfm_dataset_load_stream_csc", "nfm_transpose_file", "nfm_convert_ffm")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    assert hdr["nfm_dataset_dump_stream"][1] == ["NfmDataset", "cstring", "int64"]
    assert hdr["nfm_dataset_format_stream"][1] == ["NfmDataset", "int64", "cstring", "int64", "ptr int64"]
    assert hdr["nfm_dataset_load_stream_csc"][1] == hdr["nfm_dataset_load_stream"][1] == ["NfmCtx", "cstring", "cstring", "ptr NfmDataset"]
    assert hdr["nfm_transpose_file"][1] == ["NfmCtx", "cstring", "cstring", "int64"]
    assert hdr["nfm_convert_ffm"][1] == hdr["nfm_convert_svmlight"][1] == ["NfmCtx", "cstring", "cstring", "cstring"]
    # every entry cites the reference lines it replaces
    raw = open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    for cite in ("tensor/sparse_stream.nim:3-33", "dataset.nim:176-179", "dataset.nim:1100-1199", "dataset.nim:1202-1299", ":1122-1124",
                 ":1150, 1190-1196", ":1287 against :1294", "dataset.nim:1021-1022, 1052-1053"):
        assert cite in raw, cite


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table


def test_python_names_and_the_reference_parameter_names():
    import nimfm_amd as nf
    want = {
        "newStreamCSCDataset": ["f", "fY", "ctx"],
        "transposeFile": ["fIn", "fOut", "cacheSize", "ctx", "chunkBytes"],
        "convertFFMFile": ["fIn", "fOutX", "fOutY", "ctx"],
        "dumpStreamFile": ["f", "X", "chunkBytes"],
        "formatStream": ["X", "chunkBytes"],
        "loadStreamLabel": ["fIn"],
    }
    for name, params in want.items():
        assert hasattr(nf, name), name
        assert list(inspect.signature(getattr(nf, name)).parameters) == params, name
    assert inspect.signature(nf.transposeFile).parameters["cacheSize"].default == 200  # dataset.nim:1100
    assert inspect.signature(nf.transposeFile).parameters["chunkBytes"].default == 0
    assert inspect.signature(nf.newStreamCSCDataset).parameters["fY"].default is None
    assert list(inspect.signature(nf.convertFFMFile).parameters) == list(inspect.signature(nf.convertSVMLightFile).parameters)


def test_hosts_refuse_before_any_device_call(tmp_path):
    import numpy as np

    import nimfm_amd as nf

    S = nf.StreamCSRDataset.__new__(nf.StreamCSRDataset)  # a dataset used in row blocks: no resident handle
    S.h = None
    with pytest.raises(ValueError, match="resident"):
        nf.dumpStreamFile(str(tmp_path / "x.bin"), S)
    with pytest.raises(ValueError, match="resident"):
        nf.formatStream(S)
    (tmp_path / "y.bin").write_bytes(np.array([1.5, -2.0, 0.0]).tobytes())
    assert np.array_equal(nf.loadStreamLabel(str(tmp_path / "y.bin")), [1.5, -2.0, 0.0])


def test_nim_host_procs():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_dataset.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_dataset_load_stream_csc", "nfm_dataset_dump_stream"} <= calls
    for call in calls:
        assert call in nim, "hip_dataset.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    for sig in (r'proc newHipStreamCSCDataset\*\(f: string, fY: string = ""\): HipCSCDataset',
                r"proc dumpStreamFile\*\(f: string, X: HipCSRDataset\)",
                r"proc dumpStreamFile\*\(f: string, X: HipCSCDataset\)"):
        assert re.search(sig, flat), sig
    assert "nfm_dataset_dump_stream(rowsOf(X).handle, f.cstring, 0'i64)" in flat
    assert "transposeFieldFile" not in flat  # not offered
    # no string-only proc under a name of the reference's: it would be ambiguous with dataset.nim:1100, 1202 wherever both are seen
    assert not re.search(r"proc (transposeFile|convertFFMFile|convertSVMLightFile)\*", flat)


def test_cpp_host_names():
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ('inline std::unique_ptr<CSCDataset> newStreamCSCDataset(const std::string& f, const std::string& fY = "")',
                  "inline void transposeFile(const std::string& fIn, const std::string& fOut, int cacheSize = 200, int64_t chunkBytes = 0)",
                  "inline void convertFFMFile(const std::string& fIn, const std::string& fOutX, const std::string& fOutY)",
                  "inline void dumpStreamFile(const std::string& f, const CSRDataset& X, int64_t chunkBytes = 0)",
                  "inline std::string formatStream(const CSRDataset& X, int64_t chunkBytes = 0)",
                  "inline std::vector<double> loadStreamLabel(const std::string& fIn)",
                  "nfm_dataset_load_stream_csc(default_context()", "nfm_transpose_file(default_context()", "nfm_convert_ffm(default_context()",
                  "nfm_dataset_dump_stream(X.handle()", "nfm_dataset_format_stream(X.handle()"):
        assert piece in hpp, piece


def test_docs_name_the_feature():
    for doc, words in (("README.md", ("newStreamCSCDataset", "transposeFile", "convertFFMFile")),
                       ("INTEGRATION.md", ("nfm_dataset_dump_stream", "nfm_transpose_file", "newHipStreamCSCDataset")),
                       ("DESIGN.md", ("transposeFieldFile", "stream_pieces.h", "k_pack_stream"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
