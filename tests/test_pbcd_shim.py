"""CPU: the Nim side of proximal block coordinate descent (nim/hip_pbcd.nim) held to include/nimfm_hip.h like the PCD shim
(tests/test_pcd_shim.py): hip_pbcd.nim calls only entry points that nim/nimfm_hip.nim declares, the PBCD declaration matches
the header, and the fit overload carries the reference's signature (optimizer/pbcd.nim:212-214)."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos


def test_pbcd_declaration_matches_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert "nfm_pbcd_create" in hdr and "nfm_pbcd_create" in nim
    assert nim["nfm_pbcd_create"] == hdr["nfm_pbcd_create"], (nim["nfm_pbcd_create"], hdr["nfm_pbcd_create"])


def test_hip_pbcd_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_pbcd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_pbcd_create", "nfm_cd_begin_fit", "nfm_opt_epoch"} <= calls
    for call in calls:
        assert call in nim, "hip_pbcd.nim calls %s, which nimfm_hip.nim does not declare" % call


def test_fit_overload_on_the_device_dataset():
    flat = " ".join(open(os.path.join(NIM, "hip_pbcd.nim")).read().split())
    assert re.search(r"proc fit\*\[L, R\]\(self: PBCD\[L, R\], X: HipCSRDataset, y: seq\[float64\], sfm: FactorizationMachine, "
                     r"callback: \(PBCD\[L, R\], FactorizationMachine\)->void = nil\)", flat)
    # the verbose line before the callback (pbcd.nim:302-314), with the unscaled strengths (:303-306)
    assert flat.index("echoInfo(") < flat.index("callback(self, sfm)") and "viol < self.tol" in flat
    assert "regularization(sfm.P, sfm.w, sfm.intercept, self.alpha0, self.alpha, self.beta)" in flat
    # maxSearch != 0 and shuffle are refused before anything runs
    assert flat.index("self.maxSearch != 0") < flat.index("nfm_pbcd_create(") > flat.index("self.shuffle")


def test_integration_names_the_include():
    doc = open(os.path.join(os.path.dirname(NIM), "INTEGRATION.md")).read()
    assert "nim/hip_pbcd.nim" in doc and "include hip_pbcd" in doc
