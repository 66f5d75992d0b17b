"""CPU: the Nim side of coordinate descent (nim/hip_cd.nim) held to include/nimfm_hip.h like the other shims
(tests/test_nim_shim.py checks the FFI block, but not a new include file): hip_cd.nim calls only entry points that
nim/nimfm_hip.nim declares, the CD declarations match the header, and the fit overload carries the reference's name."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos


def test_cd_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ("nfm_cd_create", "nfm_cd_begin_fit", "nfm_cd_schedule"):
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])


def test_hip_cd_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_cd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert {"nfm_cd_create", "nfm_cd_begin_fit", "nfm_opt_epoch"} <= calls
    for call in calls:
        assert call in nim, "hip_cd.nim calls %s, which nimfm_hip.nim does not declare" % call


def test_fit_overload_on_the_device_dataset():
    flat = " ".join(open(os.path.join(NIM, "hip_cd.nim")).read().split())
    assert re.search(r"proc fit\*\[L\]\(self: CD\[L\], X: HipCSRDataset, y: seq\[float64\], fm: FactorizationMachine, callback:", flat)
    assert "callback(self, fm)" in flat and "viol < self.tol" in flat


def test_integration_names_the_include():
    doc = open(os.path.join(os.path.dirname(NIM), "INTEGRATION.md")).read()
    assert "nim/hip_cd.nim" in doc and "include hip_cd" in doc
