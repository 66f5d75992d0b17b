"""The two entry points of the seen-items mask and the ranking metrics across the header, the binding, the Nim files and nimfm.hpp
(DESIGN.md section 32), as tests/test_cross_shim.py holds the first three.  No GPU."""
import os
import re

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = {
    "nfm_cross_topk_seen": ["NfmModel", "NfmDataset", "NfmDataset", "NfmDataset", "int64", "int64", "ptr int64", "ptr float64"],
    "nfm_cross_rank_metrics": ["NfmModel", "NfmDataset", "NfmDataset", "NfmDataset", "NfmDataset", "int64", "int64", "ptr float64"],
}


def test_declarations_match_the_header_and_the_binding():
    from nimfm_amd import _capi
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = open(_capi.__file__).read()
    for name, args in ENTRIES.items():
        assert nim[name] == hdr[name] and hdr[name][1] == args, (name, nim.get(name), hdr.get(name))
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table


def test_nim_and_cpp_hosts():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    flat = " ".join(re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_cross.nim")).read()).split())
    assert {"nfm_cross_topk_seen", "nfm_cross_rank_metrics"} <= set(re.findall(r"\b(nfm_\w+)\(", flat)) <= set(nim)
    assert "proc recommend*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, seen: HipCSRDataset, topK: int, chunkItems: int = 0)" in flat
    assert ("proc rankingScore*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, heldOut: HipCSRDataset, topK: int, "
            "seen: HipCSRDataset = nil, chunkItems: int = 0): RankingScore") in flat
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("recommend(const CSRDataset& U, const CSRDataset& V, const CSRDataset& seen, int64_t topK, int64_t chunkItems = 0)",
                  "RankingScore rankingScore(const CSRDataset& U, const CSRDataset& V, const CSRDataset& heldOut, int64_t topK, const CSRDataset* seen = nullptr, "
                  "int64_t chunkItems = 0)",
                  "nfm_cross_topk_seen(push(), U.handle(), V.handle(), seen.handle(), topK, chunkItems",
                  "nfm_cross_rank_metrics(push(), U.handle(), V.handle(), seen ? seen->handle() : nullptr, heldOut.handle(), topK, chunkItems, out)"):
        assert piece in hpp, piece
