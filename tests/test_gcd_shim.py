"""The Nim side of GreedyCD (nim/hip_gcd.nim and its declarations in nim/nimfm_hip.nim) cannot be compiled here, so it is held
to include/nimfm_hip.h mechanically, as tests/test_hazan_shim.py holds Hazan's file.  No GPU."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos

ENTRIES = ("nfm_gcd_create", "nfm_gcd_begin_fit", "nfm_gcd_outer_begin", "nfm_gcd_inner", "nfm_gcd_outer_end")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])


def test_the_include_file_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_gcd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRIES) <= calls and "nfm_opt_epoch" not in calls and "nfm_hazan_iter" not in calls
    for call in calls:
        assert call in nim, "hip_gcd.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    assert re.search(r"proc fit\*\[L\]\(self: GreedyCD\[L\], X: HipCSRDataset, y: seq\[float64\], cfm: ConvexFactorizationMachine, callback:", flat)
    assert "2*rand(1.0) - 1.0" in flat and "callback(self, cfm)" in flat and "mod self.nRefitting == 0" in flat
    # the start vector is drawn only while a base is added, and the draw is what decides the argument
    assert re.search(r"let addBase = nComponents < cfm.maxComponents if addBase: for j in 0\.\.<nFeatures: start\[j\] = 2\*rand\(1.0\) - 1.0", flat)
    assert "Outer Iteration {it+1}" in flat and "Objective did not converge. Increase maxIter." in flat


def test_the_record_matches_the_header():
    _, h = header_protos()
    names = re.search(r"enum \{ (NFM_GCD_REC_ADDED.*?) \};", h, flags=re.S).group(1)
    rec = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in names.replace("\n", " ").split(",")))
    from nimfm_amd import _capi
    assert rec["NFM_GCD_REC_COUNT"] == 8 == len(_capi.GCD_REC)
    order = ["ADDED", "SLOT", "LAM", "POWER_ITERS", "EVAL", "N_COMPONENTS", "OBJECTIVE", "N_STORED"]
    assert [rec["NFM_GCD_REC_" + k] for k in order] == list(range(8))
    assert [k.lower().replace("_", "") for k in order] == [k.lower() for k in _capi.GCD_REC]
    # the hosts read the record by these positions
    src = open(os.path.join(NIM, "hip_gcd.nim")).read()
    assert "rec[5].int" in src and "rec[6]" in src and "rec[0] != 0.0" in src


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table
