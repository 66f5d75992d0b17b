"""CPU: the Nim side of PGD, FISTA and NMAPGD (nim/hip_pgd.nim) held to include/nimfm_hip.h like the PBCD shim
(tests/test_pbcd_shim.py): hip_pgd.nim calls only entry points that nim/nimfm_hip.nim declares, the three declarations match
the header, and the fit overloads carry the reference's signatures (optimizer/pgd.nim:149-151, fista.nim:52-54,
nmapgd.nim:174-176)."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos

ENTRY = ("nfm_pgd_create", "nfm_pgd_begin_fit", "nfm_pgd_last_iter")


def test_pgd_declarations_match_the_header():
    hdr, h = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRY:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    # the record hip_pgd.nim reads is as long as the header says
    count = int(re.search(r"NFM_PGD_IT_COUNT\s*=\s*(\d+)", h).group(1))
    src = open(os.path.join(NIM, "hip_pgd.nim")).read()
    assert "array[%d, float64]" % count in src


def test_hip_pgd_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_pgd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRY) | {"nfm_opt_epoch"} <= calls
    for call in calls:
        assert call in nim, "hip_pgd.nim calls %s, which nimfm_hip.nim does not declare" % call


def test_fit_overloads_on_the_device_dataset():
    flat = " ".join(open(os.path.join(NIM, "hip_pgd.nim")).read().split())
    for name in ("PGD", "FISTA", "NMAPGD"):
        assert re.search(r"proc fit\*\[L, R\]\(self: %s\[L, R\], X: HipCSRDataset, y: seq\[float64\], sfm: FactorizationMachine, "
                         r"callback: \(%s\[L, R\], FactorizationMachine\)->void = nil\)" % (name, name), flat), name
    # the callback before the verbose line, the stopping test on viol, PGD's `epoch` against the others' `it+1`
    assert flat.index("callback(self, sfm)") < flat.index("echoInfo(") and "viol < self.tol" in flat
    assert "hipPgdFit(self, 0, 0.5, 0," in flat and "hipPgdFit(self, 1, 0.5, 1," in flat and "hipPgdFit(self, 2, self.eta, 1," in flat
    assert "self.reg.initSGD(" in flat and flat.index("self.reg.initSGD(") < flat.index("nfm_pgd_create(")


def test_integration_names_the_include():
    doc = open(os.path.join(os.path.dirname(NIM), "INTEGRATION.md")).read()
    assert "nim/hip_pgd.nim" in doc and "include hip_pgd" in doc
