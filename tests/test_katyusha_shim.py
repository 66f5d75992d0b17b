"""The Nim side of Katyusha (nim/hip_katyusha.nim and its declarations in nim/nimfm_hip.nim) cannot be compiled here, so it is
held to include/nimfm_hip.h mechanically, as tests/test_nim_shim.py holds the other solvers' files.  No GPU."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos

ENTRIES = ("nfm_katyusha_create", "nfm_katyusha_begin_fit", "nfm_katyusha_snapshot")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])


def test_the_include_file_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_katyusha.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRIES) <= calls and "nfm_opt_epoch" in calls
    for call in calls:
        assert call in nim, "hip_katyusha.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    assert re.search(r"proc fit\*\[L, R\]\(self: Katyusha\[L, R\], X: HipCSRDataset, y: seq\[float64\], sfm: FactorizationMachine, callback:", flat)
    assert "nCalls > 0" in flat and "callback(self, sfm)" in flat


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table
