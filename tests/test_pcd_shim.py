"""CPU: the Nim side of proximal coordinate descent (nim/hip_pcd.nim) held to include/nimfm_hip.h like the CD shim
(tests/test_cd_shim.py): hip_pcd.nim calls only entry points that nim/nimfm_hip.nim declares, the PCD declaration matches
the header, and the fit overload carries the reference's signature (optimizer/pcd.nim:110-112)."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos


def test_pcd_declaration_matches_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    assert "nfm_pcd_create" in hdr and "nfm_pcd_create" in nim
    assert nim["nfm_pcd_create"] == hdr["nfm_pcd_create"], (nim["nfm_pcd_create"], hdr["nfm_pcd_create"])


def test_hip_pcd_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_pcd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_pcd_create", "nfm_cd_begin_fit", "nfm_opt_epoch"} <= calls
    for call in calls:
        assert call in nim, "hip_pcd.nim calls %s, which nimfm_hip.nim does not declare" % call


def test_fit_overload_on_the_device_dataset():
    flat = " ".join(open(os.path.join(NIM, "hip_pcd.nim")).read().split())
    assert re.search(r"proc fit\*\[L, R\]\(self: PCD\[L, R\], X: HipCSRDataset, y: seq\[float64\], sfm: FactorizationMachine, "
                     r"callback: \(PCD\[L, R\], FactorizationMachine\)->void = nil\)", flat)
    # the verbose line before the callback (pcd.nim:188-192)
    assert flat.index("echoInfo(") < flat.index("callback(self, sfm)") and "viol < self.tol" in flat


def test_integration_names_the_include():
    doc = open(os.path.join(os.path.dirname(NIM), "INTEGRATION.md")).read()
    assert "nim/hip_pcd.nim" in doc and "include hip_pcd" in doc
