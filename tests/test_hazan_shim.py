"""The Nim side of the convex factorization machine and Hazan (nim/hip_hazan.nim and its declarations in nim/nimfm_hip.nim)
cannot be compiled here, so it is held to include/nimfm_hip.h mechanically, as tests/test_katyusha_shim.py holds Katyusha's
file.  No GPU."""
import os
import re

from test_nim_shim import NIM, header_protos, nim_protos

ENTRIES = ("nfm_cfm_create", "nfm_cfm_set_params", "nfm_cfm_get_params", "nfm_hazan_create", "nfm_hazan_begin_fit", "nfm_hazan_iter",
           "nfm_rng_rand_uniform")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])


def test_the_include_file_calls_only_declared_entry_points():
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_hazan.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRIES) - {"nfm_rng_rand_uniform"} <= calls and "nfm_decision_function" in calls and "nfm_opt_epoch" not in calls
    for call in calls:
        assert call in nim, "hip_hazan.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    assert re.search(r"proc fit\*\(self: Hazan, X: HipCSRDataset, y: seq\[float64\], cfm: ConvexFactorizationMachine, callback:", flat)
    assert "proc decisionFunction*(self: ConvexFactorizationMachine, X: HipCSRDataset): seq[float64]" in flat
    assert "2*rand(1.0) - 1.0" in flat and "callback(self, cfm)" in flat and "inc(self.it)" in flat


def test_the_record_matches_the_header():
    _, h = header_protos()
    names = re.search(r"enum \{ (NFM_HAZAN_REC_LOSS.*?) \};", h, flags=re.S).group(1)
    rec = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in names.replace("\n", " ").split(",")))
    assert rec["NFM_HAZAN_REC_COUNT"] == 8 and rec["NFM_HAZAN_REC_LOSS"] == 0 and rec["NFM_HAZAN_REC_TRACE"] == 1
    assert rec["NFM_HAZAN_REC_N_COMPONENTS"] == 7
    from nimfm_amd import _capi
    assert len(_capi.HAZAN_REC) == rec["NFM_HAZAN_REC_COUNT"]
    order = ["LOSS", "TRACE", "SLOT", "STEP", "POWER_ITERS", "CG_ITERS", "EVAL", "N_COMPONENTS"]
    assert [rec["NFM_HAZAN_REC_" + k] for k in order] == list(range(8))
    assert [k.lower().replace("_", "") for k in order] == [k.lower() for k in _capi.HAZAN_REC]


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table
