"""The entry point of sampleCandidates across the header, the binding, the Nim files and nimfm.hpp, as
tests/test_cross_seen_shim.py holds the ranking entry points.  No GPU."""
import os
import re

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ARGS = ["NfmDataset", "NfmDataset", "int64", "int64", "ptr NfmDataset"]


def test_declarations_match_the_header_and_the_binding():
    from nimfm_amd import _capi
    import nimfm_amd as nf
    hdr, text = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert nim["nfm_sample_candidates"] == hdr["nfm_sample_candidates"] == ("int32", ARGS)
    assert open(_capi.__file__).read().count('"nfm_sample_candidates"') == 2  # the symbol list and the signature table
    cand_max = re.search(r"kCandMax = (\d+);", open(os.path.join(ROOT, "nimfm_amd", "csrc", "candidates.h")).read()).group(1)
    assert nf.kCandMax == int(cand_max) and "n_per_user <= %s" % cand_max in open(os.path.join(ROOT, "include", "nimfm_hip.h")).read()
    assert callable(nf.sampleCandidates)


def test_nim_and_cpp_hosts():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    flat = " ".join(re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_cross.nim")).read()).split())
    assert "nfm_sample_candidates" in set(re.findall(r"\b(nfm_\w+)\(", flat)) <= set(nim)
    assert "proc sampleCandidates*(exclude: HipCSRDataset, nPerUser: int, seed: uint64, includeSet: HipCSRDataset = nil): HipCSRDataset" in flat
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    for piece in ("inline CSRDataset sampleCandidates(const CSRDataset& exclude, int64_t nPerUser, uint64_t seed, const CSRDataset* include = nullptr)",
                  "nfm_sample_candidates(exclude.handle(), include ? include->handle() : nullptr, nPerUser, (int64_t)seed, &h)"):
        assert piece in hpp, piece
