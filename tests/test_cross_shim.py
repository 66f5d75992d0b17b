"""crossDecisionFunction / recommend across the three hosts: the three entry points of include/nimfm_hip.h
against nimfm_amd/_capi.py, nim/nimfm_hip.nim and nimfm_amd/host/nimfm.hpp, and the two procs with their signatures
(nim/hip_cross.nim cannot be compiled here, so it is held to the header mechanically, as tests/test_stream_csc_shim.py does).
No GPU."""
import inspect
import os
import re

import pytest

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = ("nfm_cross_decision_function", "nfm_cross_decision_function_device", "nfm_cross_topk")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    assert hdr["nfm_cross_decision_function"][1] == ["NfmModel", "NfmDataset", "NfmDataset", "ptr float64"]
    assert hdr["nfm_cross_decision_function_device"][1] == ["NfmModel", "NfmDataset", "NfmDataset", "ptr float64"]
    assert hdr["nfm_cross_topk"][1] == ["NfmModel", "NfmDataset", "NfmDataset", "int64", "int64", "ptr int64", "ptr float64"]


def test_every_prototype_cites_the_reference():
    raw = open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    for name in ENTRIES:
        at = raw.index("int32_t %s(" % name)
        comment = raw[raw.rindex("/*", 0, at):at]
        assert comment.rstrip().endswith("*/"), name  # the comment directly above the prototype
        for cite in ("factorization_machine.nim:100-122", "kernels.nim:59-64", "tensor/sparse.nim:671-698"):
            assert cite in comment, (name, cite)


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table


def test_python_host_signatures():
    import nimfm_amd as nf
    assert list(inspect.signature(nf.FactorizationMachine.crossDecisionFunction).parameters) == ["self", "U", "V"]
    sig = inspect.signature(nf.FactorizationMachine.recommend)
    assert list(sig.parameters) == ["self", "U", "V", "topK", "chunkItems"] and sig.parameters["chunkItems"].default == 0
    # on FactorizationMachine alone: the other model kinds have no such call (the library refuses their handles)
    for other in (nf.FieldAwareFactorizationMachine, nf.ConvexFactorizationMachine):
        assert not hasattr(other, "crossDecisionFunction") and not hasattr(other, "recommend")
    from cross_cases import tile_shape
    t = tile_shape()
    assert set(t) == {"TU", "TV", "KS", "maxTopK"} and t["maxTopK"] == 256 and all(v > 0 for v in t.values())


def test_python_host_refuses_before_any_device_call():
    import numpy as np

    import nimfm_amd as nf
    from nimfm_amd import _capi

    fm = nf.FactorizationMachine("r", nComponents=2)
    S = nf.StreamCSRDataset.__new__(nf.StreamCSRDataset)  # a dataset used in row blocks: no resident handle
    S.h = None
    with pytest.raises(_capi.NotFittedError):
        fm.crossDecisionFunction(S, S)
    fm.set_params(np.ones((1, 2, 4)), np.zeros(4), 0.0)
    for call in (lambda: fm.crossDecisionFunction(S, S), lambda: fm.recommend(S, S, 1)):
        with pytest.raises(_capi.NfmError, match="StreamCSRDataset") as e:
            call()
        assert e.value.code == _capi.ERR_UNSUPPORTED and "decisionFunction" in str(e.value)


def test_nim_host_procs():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    core = open(os.path.join(NIM, "nimfm_hip.nim")).read()
    assert "when defined(nimfmHip): include hip_cross" in core
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_cross.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_cross_decision_function", "nfm_cross_topk"} <= calls
    for call in calls:
        assert call in nim, "hip_cross.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    for a, b in (("HipCSRDataset", "HipCSRDataset"), ("HipCSCDataset", "HipCSCDataset"), ("HipCSCDataset", "HipCSRDataset"),
                 ("HipCSRDataset", "HipCSCDataset")):
        assert re.search(r"proc crossDecisionFunction\*\(self: FactorizationMachine, U: %s, V: %s\): seq\[seq\[float64\]\]" % (a, b), flat)
        assert re.search(r"proc recommend\*\(self: FactorizationMachine, U: %s, V: %s, topK: int, chunkItems: int = 0\): "
                         r"tuple\[ids: seq\[seq\[int\]\], scores: seq\[seq\[float64\]\]\]" % (a, b), flat)
    assert "Invalid nFeatures." in flat and "self.checkInitialized()" in flat


def test_cpp_host_members():
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("std::vector<double> crossDecisionFunction(const CSRDataset& U, const CSRDataset& V)",
                  "std::pair<std::vector<int64_t>, std::vector<double>> recommend(const CSRDataset& U, const CSRDataset& V, int64_t topK, "
                  "int64_t chunkItems = 0)",
                  "nfm_cross_decision_function(push(), U.handle(), V.handle()", "nfm_cross_topk(push(), U.handle(), V.handle(), topK, chunkItems"):
        assert piece in hpp, piece
    fm_class = hpp[hpp.index("class FactorizationMachine {"):hpp.index("class SGD {")]
    assert "crossDecisionFunction" in fm_class and "recommend" in fm_class
