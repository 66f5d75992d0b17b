"""The row-local proximal step is written out twice on purpose (nimfm_amd/csrc/prox_dev.h says why): in k_psgd_dense
(psgd.hip) and in k_pgd_trial (pgd.hip).  The two texts are the same statements once the kernels' own names for the
regulariser, lam and the norm's slot are put aside; this holds them together.  No GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nimfm_amd", "csrc")
END = "if (act) *reinterpret_cast<double2*>(M.P + e) = p;"


def _row_local_prox(name, first, renames):
    text = open(os.path.join(CSRC, name)).read()
    body = text[text.index(first):]
    body = body[:body.index(END)]
    body = re.sub(r"//[^\n]*", "", body)  # the comments differ: each cites the other copy
    for old, new in renames:
        body = body.replace(old, new)
    return re.sub(r"\s+", " ", body).strip()


def test_row_local_prox_copies_match():
    psgd = _row_local_prox("psgd.hip", "if (O.reg == NFM_REG_L1) {", [("O.reg", "reg"), ("a.norms[r]", "NORM")])
    pgd = _row_local_prox("pgd.hip", "if (a.reg == NFM_REG_L1) {",
                          [("a.reg", "reg"), ("a.lam", "lam"), ("a.norms[(size_t)b * M.da + j]", "NORM")])
    assert psgd == pgd
    for piece in ("soft_threshold(p.x, lam)", "reg == NFM_REG_L21", "NORM = nrm", "pass < 2 * L + 2", "soft_threshold(p.x, tau)"):
        assert piece in psgd, piece
