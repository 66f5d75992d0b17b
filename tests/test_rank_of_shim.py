"""The entry point of rankOf across the header, the binding, the Nim files and nimfm.hpp, as
tests/test_candidates_shim.py holds sampleCandidates.  No GPU."""
import os
import re

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ARGS = ["NfmModel", "NfmDataset", "NfmDataset", "NfmDataset", "NfmDataset", "int64", "ptr int64", "ptr int64"]


def test_declarations_match_the_header_and_the_binding():
    from nimfm_amd import _capi
    import nimfm_amd as nf
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert nim["nfm_cross_rank_of"] == hdr["nfm_cross_rank_of"] == ("int32", ARGS)
    assert open(_capi.__file__).read().count('"nfm_cross_rank_of"') == 2  # the symbol list and the signature table
    text = open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    comment = text[:text.index("int32_t nfm_cross_rank_of(")].rsplit("/*", 1)[1]  # cites the scores' lines, names no counterpart
    assert "model/factorization_machine.nim:100-122" in comment and "no counterpart" in comment
    assert callable(nf.FactorizationMachine.rankOf)


def test_nim_and_cpp_hosts():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    flat = " ".join(re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_cross.nim")).read()).split())
    assert "nfm_cross_rank_of" in set(re.findall(r"\b(nfm_\w+)\(", flat)) <= set(nim)
    assert ("proc rankOf*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, heldOut: HipCSRDataset, seen: HipCSRDataset = nil, "
            "chunkItems: int = 0): tuple[ranks: seq[int], nCandidates: seq[int]]") in flat
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("rankOf(const CSRDataset& U, const CSRDataset& V, const CSRDataset& heldOut, const CSRDataset* seen = nullptr, int64_t chunkItems = 0)",
                  "nfm_cross_rank_of(push(), U.handle(), V.handle(), heldOut.handle(), seen ? seen->handle() : nullptr, chunkItems, ranks.data(), "
                  "nCandidates.data())"):
        assert piece in hpp, piece
