"""CPU: OmegaCS's regulariser id is one number in the C header, the Python host's table and the Nim shim, and the
integration notes name the shim's overload."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_omegacs_id_is_5_everywhere():
    from nimfm_amd import _capi as capi
    assert re.search(r"\bNFM_REG_OMEGACS\s*=\s*5\b", _read("include", "nimfm_hip.h"))
    assert capi.REG["omegacs"] == 5
    assert len(set(capi.REG.values())) == len(capi.REG)
    nim = _read("nim", "hip_pbcd.nim")
    assert re.search(r"^proc pbcdRegId\(reg: OmegaCS\): int32 = 5$", nim, re.M)
    assert re.search(r"^import \.\./regularizer/regularizers$", nim, re.M)  # the module that exports the type OmegaCS


def test_integration_notes_name_omegacs():
    assert any("hip_pbcd.nim" in line and "OmegaCS" in line for line in _read("INTEGRATION.md").splitlines())
