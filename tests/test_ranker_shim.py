"""The Ranker's entry points across the header, the binding, the Nim files and nimfm.hpp, as
tests/test_cross_shim.py holds crossDecisionFunction.  No GPU."""
import inspect
import os
import re

import pytest

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = {"nfm_ranker_create": ["NfmModel", "NfmDataset", "NfmDataset", "pointer"], "nfm_ranker_destroy": ["pointer"],
           "nfm_ranker_scores": ["pointer", "ptr float64"], "nfm_ranker_scores_at": ["pointer", "NfmDataset", "ptr float64"],
           "nfm_ranker_topk": ["pointer", "int64", "NfmDataset", "int64", "ptr int64", "ptr float64"],
           "nfm_ranker_rank_of": ["pointer", "NfmDataset", "NfmDataset", "int64", "ptr int64", "ptr int64"]}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_declarations_agree_and_cite_the_reference(name):
    from nimfm_amd import _capi
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert nim[name] == hdr[name] == ("int32", ENTRIES[name])
    assert open(_capi.__file__).read().count('"%s"' % name) == 2  # the symbol list and the signature table
    raw = open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    at = raw.index("int32_t %s(" % name)
    comment = raw[raw.rindex("/*", 0, at):at]
    assert comment.rstrip().endswith("*/") and ("field_aware_factorization_machine.nim:52-76" in comment or "no counterpart" in comment)


def test_hosts():
    import nimfm_amd as nf
    assert list(inspect.signature(nf.newRanker).parameters) == ["model", "U", "V"]
    for meth, params in (("scores", []), ("scoresAt", ["pairs"]), ("recommend", ["topK", "seen", "chunkItems"]), ("rankOf", ["heldOut", "seen", "chunkItems"])):
        assert list(inspect.signature(getattr(nf.Ranker, meth)).parameters) == ["self"] + params
    nim, core = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert "when defined(nimfmHip): include hip_ranker" in core
    flat = " ".join(re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_ranker.nim")).read()).split())
    assert set(ENTRIES) <= set(re.findall(r"\b(nfm_\w+)\(", flat)) <= set(nim)
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("proc newRanker*(self: FactorizationMachine,", "proc newRanker*(self: FieldAwareFactorizationMachine,", "proc scores*(self: Ranker)",
                  "proc scoresAt*(self: Ranker,", "proc recommend*(self: Ranker,", "proc rankOf*(self: Ranker,"):
        assert piece in flat, piece
    for piece in ("class Ranker {", "nfm_ranker_create(fm.push(), U.handle(), V.handle(), &h_)", "nfm_ranker_topk(h_, topK,", "nfm_ranker_rank_of(h_,",
                  "nfm_ranker_scores_at(h_,", "nfm_ranker_scores(h_,"):
        assert piece in hpp, piece


def test_python_host_refuses_before_any_device_call():
    import numpy as np

    import nimfm_amd as nf
    from nimfm_amd import _capi
    ffm = nf.FieldAwareFactorizationMachine("r", nComponents=2)
    S = nf.StreamCSRDataset.__new__(nf.StreamCSRDataset)  # a dataset used in row blocks: no resident handle
    with pytest.raises(_capi.NotFittedError):
        nf.newRanker(ffm, S, S)
    ffm.set_params(np.ones((2, 4, 2)), np.zeros(4), 0.0)
    with pytest.raises(_capi.NfmError, match="StreamCSRDataset") as e:
        nf.newRanker(ffm, S, S)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "decisionFunction" in str(e.value)
