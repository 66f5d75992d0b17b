"""The Nim side of PSGD (nim/hip_psgd.nim and its declarations in nim/nimfm_hip.nim) cannot be compiled here, so it is held to
include/nimfm_hip.h mechanically, as tests/test_gcd_shim.py holds GreedyCD's file.  No GPU."""
import os
import re

from test_nim_shim import NIM, ROOT, header_protos, nim_protos

ENTRIES = ("nfm_psgd_create", "nfm_psgd_begin_fit", "nfm_psgd_finalize")


def test_declarations_match_the_header():
    hdr, _ = header_protos()
    nim, _ = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    for name in ENTRIES:
        assert name in hdr and name in nim, name
        assert nim[name] == hdr[name], (name, nim[name], hdr[name])
    assert hdr["nfm_psgd_create"][1] == ["NfmModel", "ptr NfmMbpsgdCfg", "ptr NfmOpt"]  # newMBPSGD's config object


def test_the_include_file_calls_only_declared_entry_points():
    nim, core = nim_protos(os.path.join(NIM, "nimfm_hip.nim"))
    src = re.sub(r"##.*|#.*", "", open(os.path.join(NIM, "hip_psgd.nim")).read())
    calls = set(re.findall(r"\b(nfm_\w+)\(", src))
    assert set(ENTRIES) <= calls and {"nfm_opt_epoch", "nfm_opt_set_it"} <= calls and "nfm_mbpsgd_create" not in calls
    assert "nfm_opt_finalize" not in calls  # finalize is the solver's own entry
    for call in calls:
        assert call in nim, "hip_psgd.nim calls %s, which nimfm_hip.nim does not declare" % call
    flat = " ".join(src.split())
    assert re.search(r"proc fit\*\[L, R\]\(self: PSGD\[L, R\], X: HipCSRDataset, y: seq\[float64\], sfm: FactorizationMachine, callback:", flat)
    # begin_fit before the first epoch call, finalize before every callback and at the end, the reference's loop pieces
    assert flat.index("nfm_psgd_begin_fit(") < flat.index("nfm_opt_epoch(")
    assert flat.count("nfm_psgd_finalize(o)") == 3 and flat.count("callback(self, sfm)") == 2
    assert "mod self.nCalls == 0" in flat and "echoHeader(self.maxIter, viol=false)" in flat
    assert "abs(runningLoss - runningLossOld) < self.tol" in flat and "Objective did not converge. Increase maxIter." in flat
    assert "self.gamma * self.reg.eval(" in flat and "if not sfm.warmStart: self.it = 1" in flat
    # only L1 and L21 have an id; everything else raises and names newMBPSGD
    assert "proc psgdRegId(reg: L1): int32 = 0" in flat and "proc psgdRegId(reg: L21): int32 = 1" in flat and "newMBPSGD" in flat
    assert "include hip_psgd" in core
    assert "hip_psgd.nim" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_three_hosts_agree_on_names_and_defaults():
    """newPSGD's parameters and defaults (psgd.nim:23-27) in the Python host and the C++ host"""
    import inspect

    import nimfm_amd as nf
    sig = inspect.signature(nf.newPSGD)
    want = dict(maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, scheduling="optimal",
                power=1.0, verbose=1, tol=1e-3, shuffle=True, nCalls=-1)
    got = {k: v.default for k, v in sig.parameters.items() if v.kind is not inspect.Parameter.VAR_KEYWORD}
    assert got == want and list(got) == list(want)
    assert isinstance(nf.newPSGD(verbose=0).reg, nf.SquaredL12)  # the reference's default, refused at fit
    hpp = " ".join(open(os.path.join(ROOT, "nimfm_amd", "host", "nimfm.hpp")).read().split())
    assert ("explicit PSGD(int maxIter_ = 100, double eta0_ = 0.01, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, "
            "double gamma_ = 1e-4, L loss_ = L(), R reg_ = R(), SchedulingKind scheduling_ = optimal, double power_ = 1.0, "
            "int verbose_ = 1, double tol_ = 1e-3, bool shuffle_ = true, int nCalls_ = -1)") in hpp
    assert "template <class L = Squared, class R = SquaredL12> class PSGD" in hpp


def test_python_binding_declares_the_entries():
    from nimfm_amd import _capi
    src = open(_capi.__file__).read()
    for name in ENTRIES:
        assert src.count('"%s"' % name) == 2, name  # the symbol list and the signature table


def test_default_constructed_solver_is_refused_before_any_device_call():
    """newPSGD()'s default regulariser is SquaredL12: fit raises ValueError and names newMBPSGD, without touching X"""
    import pytest

    import nimfm_amd as nf
    fm = nf.newFactorizationMachine("regression")
    with pytest.raises(ValueError, match="newMBPSGD"):
        nf.newPSGD(verbose=0).fit(None, None, fm)
    with pytest.raises(ValueError, match="no SGD hooks"):
        nf.newPSGD(verbose=0, reg=nf.newOmegaCS()).fit(None, None, fm)
    with pytest.raises(ValueError, match="devices"):
        nf.newPSGD(verbose=0, reg=nf.newL1()).fit(None, None, fm, devices=[0, 1])
    with pytest.raises(ValueError, match="nComponents <= 128"):
        nf.newPSGD(verbose=0, reg=nf.newL21()).fit(None, None, nf.newFactorizationMachine("regression", nComponents=200))
