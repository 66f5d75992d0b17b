"""interactionStats / topInteractions across the header, the binding, the Nim files and nimfm.hpp, as
tests/test_ranker_shim.py holds the Ranker.  No GPU."""
import inspect
import os
import re
import subprocess

import pytest

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = {"nfm_model_interaction_stats": ["NfmModel", "int32", "ptr float64", "ptr int64"],
           "nfm_model_top_interactions": ["NfmModel", "int32", "int64", "ptr int64", "ptr float64"]}


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
    assert comment.rstrip().endswith("*/") and "benchmarks/ml100k/utils.nim" in comment


def test_hosts():
    import nimfm_amd as nf
    assert list(inspect.signature(nf.FactorizationMachine.interactionStats).parameters) == ["self", "order"]
    assert list(inspect.signature(nf.FactorizationMachine.topInteractions).parameters) == ["self", "K", "order"]
    assert list(inspect.signature(nf.countInteractions).parameters) == list(inspect.signature(nf.countFeatures).parameters) == ["fm", "order"]
    with pytest.raises(nf.NotFittedError):
        nf.FactorizationMachine("r").interactionStats()
    nim, core = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert "when defined(nimfmHip): include hip_interactions" in core
    flat = " ".join(re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_interactions.nim")).read()).split())
    assert set(ENTRIES) <= set(re.findall(r"\b(nfm_\w+)\(", flat)) <= set(nim)
    for piece in ("proc interactionStats*(self: FactorizationMachine, order: int = 0)", "proc topInteractions*(self: FactorizationMachine, K: int, order: int = 0)",
                  "proc countInteractions*(self: FactorizationMachine,", "proc countFeatures*(self: FactorizationMachine,"):
        assert piece in flat, piece


def test_cpp_members_compile(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "nimfm.hpp"\nint main() { nimfm::FactorizationMachine fm(nimfm::regression, 3);\n'
                   '  if (fm.isInitialized) { auto s = fm.interactionStats(1); auto t = fm.topInteractions(7, 1);\n'
                   '    return (int)(s.nInteractions + s.nFeatures + s.nNonzeroRows + s.l1Norm + s.l1OffDiag) + (int)t.first.size() + (int)t.second.size(); }\n'
                   '  return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "nimfm_amd", "host"), str(src)])
