"""The row-local proximal step (L1, L21, the SquaredL21 norms, the row-wise SquaredL12 threshold iteration) has ONE definition,
NFM_ROW_LOCAL_PROX in nimfm_amd/csrc/prox_dev.h (a macro: the header says why), and k_psgd_dense (psgd.hip), k_pgd_trial
(pgd.hip) and k_kat_dense (katyusha.hip) each use it once.  No GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")
USERS = ("psgd.hip", "pgd.hip", "katyusha.hip")
# statements of the step.  The L21 factor is matched as the whole statement: pbcd.hip has the expression 1.0 - lam / nrm too, in
# the block step of one feature's row (l21.nim:25-29), which is not this pass over all rows
MARKERS = ("pass < 2 * L + 2", "soft_threshold(p.x, tau)", "const double f = nrm > lam ? 1.0 - lam / nrm : 0.0;")


def _code(name):
    """the file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_row_local_prox_has_one_definition():
    code = {name: _code(name) for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip"))}
    for marker in MARKERS:
        assert {name: text.count(marker) for name, text in code.items() if marker in text} == {"prox_dev.h": 1}, marker
    assert [name for name, text in code.items() if "#define NFM_ROW_LOCAL_PROX(" in text] == ["prox_dev.h"]
    for name, text in code.items():
        assert text.count("NFM_ROW_LOCAL_PROX(") == (1 if name in USERS + ("prox_dev.h",) else 0), name
    for name in USERS:
        assert "1.0 - lam / nrm" not in code[name] and "row_sum<L>((ax > tau" not in code[name], name
    # the shared text: what follows the #define, its line continuations folded
    shared = code["prox_dev.h"]
    shared = shared[shared.index("#define NFM_ROW_LOCAL_PROX("):]
    assert shared.startswith("#define NFM_ROW_LOCAL_PROX(L, reg, reg_transpose, lam, p, act, l, norm_slot)")
    shared = re.sub(r"\s+", " ", shared.replace("\\\n", " "))
    for piece in ("soft_threshold(p.x, lam)", "soft_threshold(p.y, lam)", "reg == NFM_REG_L21", "act && l == 0", "norm_slot = nrm",
                  "reg == NFM_REG_SQUAREDL12 && !reg_transpose", "pass < 2 * L + 2", "soft_threshold(p.x, tau)", "soft_threshold(p.y, tau)"):
        assert piece in shared, piece


def test_each_kernel_names_its_own_regulariser_lam_and_norm_slot():
    want = {"psgd.hip": "NFM_ROW_LOCAL_PROX(L, O.reg, O.reg_transpose, lam, p, act, l, a.norms[r]);",
            "pgd.hip": "NFM_ROW_LOCAL_PROX(L, a.reg, a.reg_transpose, a.lam, p, act, l, a.norms[(size_t)b * M.da + j]);",
            "katyusha.hip": "NFM_ROW_LOCAL_PROX(L, a.reg, a.reg_transpose, lam, p, act, l, a.norms[(size_t)b * M.da + j]);"}
    for name, call in want.items():
        assert call in _code(name), name
