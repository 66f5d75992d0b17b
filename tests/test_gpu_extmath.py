"""-m gpu: matmul, mvmul, vmmul of a resident dataset (nimfm_amd/csrc/extmath.hip) against the reference's
loop nests (extmath.nim:10-133) restated elementwise in numpy float64, by bytes: every element is one chain of
`acc = acc + (a * b)` in the order the storage fixes, and the library is built without contraction.

One S of 70 x 37 (more than one wavefront of rows at one lane per row): an empty row, an empty column, a row that stores a column
id twice, and one row of 600 entries -- the staging buffer of a wavefront holds kSpmmStage = 256 entries, so that row is
staged three times (two refills).  The CSCDataset holds the same entries in another, unsorted storage order.  r (m for D . S)
runs over 1, 2, 3, 64, 130 -- one lane per row, a half-full last word, a full team of 64 lanes, two words per lane with a ragged
last one -- and 513, the smallest width that needs a second column panel (a panel is 64 lanes x kSpmmAcc = 4 words x 2)."""
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import nimfm_amd as nf
from nimfm_amd import _capi as capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NF, LONG = 70, 37, 600
CASES = [(call, r) for call in ("sd", "ds") for r in (1, 2, 3, 64, 130, 513)] + [("mvmul", 1), ("vmmul", 1)]


@pytest.fixture(scope="module")
def S():
    rs = np.random.RandomState(7)
    ent, stored = [], np.delete(np.arange(NF), 11)  # column 11 stays empty
    for i in range(N):
        cols = rs.choice(stored, rs.randint(1, 13), replace=False)
        if i == 5:
            cols = []  # the empty row
        elif i == 7:
            cols = [3, 30, 3, 8]  # column 3 twice
        elif i == 20:
            cols = rs.choice(stored, LONG)
        ent += [(i, int(j)) for j in cols]
    ent, val = np.array(ent, dtype=np.int64), rs.randn(len(ent))
    ptr = lambda ids, n: np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n))]).astype(np.int64)
    shuffled = rs.permutation(len(ent))
    by_col = shuffled[np.argsort(ent[shuffled, 1], kind="stable")]  # grouped by column, the samples of a column in no order
    csr = nf.newCSRDataset(val, ent[:, 1], ptr(ent[:, 0], N), N, NF)
    csc = nf.newCSCDataset(val[by_col], ent[by_col, 0], ptr(ent[:, 1], NF), N, NF)
    # (row, column, value) of every entry in the storage order of each layout
    return SimpleNamespace(ds=dict(csr=csr, csc=csc),
                           entries=dict(csr=(ent[:, 0], ent[:, 1], val), csc=(ent[by_col, 0], ent[by_col, 1], val[by_col])))


def dense(rows, cols):
    return np.random.RandomState(1000 * rows + cols).randn(rows, cols)


def expected(S, layout, call, D):
    """The reference's loops over the layout's own storage, one entry at a time (a CSRDataset: extmath.nim:19-22, 49-52, 87-90,
    110-112; a CSCDataset: :34-37, 64-67, 99-101, 120-123); elementwise numpy keeps each element's chain and rounding."""
    if call in ("sd", "mvmul"):
        R = np.zeros((N, D.shape[1]))
        for i, j, v in zip(*S.entries[layout]):
            R[i, :] = R[i, :] + v * D[j, :]
    else:
        R = np.zeros((D.shape[0], NF))
        for i, j, v in zip(*S.entries[layout]):
            R[:, j] = R[:, j] + D[:, i] * v
    return R


def run(ds, call, D):
    if call == "sd":
        return nf.matmul(ds, D)
    if call == "ds":
        return nf.matmul(D, ds)
    return nf.mvmul(ds, D[:, 0])[:, None] if call == "mvmul" else nf.vmmul(D[0], ds)[None, :]


def operand(call, r):
    return dense(NF, r) if call in ("sd", "mvmul") else dense(r, N)


@pytest.mark.parametrize("call,r", CASES)
@pytest.mark.parametrize("layout", ["csr", "csc"])
def test_same_bytes_as_the_reference_loops(S, layout, call, r):
    D = operand(call, r)
    got, want = run(S.ds[layout], call, D), expected(S, layout, call, D)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("r", [1, 3, 64, 130])
def test_a_row_keeps_its_bits_wherever_it_stands(S, r):
    perm = np.random.RandomState(3).permutation(N)
    D = dense(NF, r)
    assert nf.matmul(S.ds["csr"][perm], D).tobytes() == np.ascontiguousarray(nf.matmul(S.ds["csr"], D)[perm]).tobytes()


@pytest.mark.parametrize("layout,call,shape,message", [
    ("csr", "sd", (NF - 1, 4), "S.shape[1] 37 != D.shape[0] 36."),
    ("csc", "sd", (NF + 1, 4), "S.shape[1] 37 != D.shape[0] 38."),
    ("csr", "ds", (4, N - 1), "D.shape[1] 69 != shape[0] 70."),
    ("csc", "ds", (4, N - 1), "D.shape[1] 69 != S.shape[0] 70."),
    ("csr", "mvmul", (NF - 1, 1), "shape[1] 37 != len(vec)36."),
    ("csc", "mvmul", (NF - 1, 1), "shape[1] 37 != len(vec)36."),
    ("csr", "vmmul", (1, N + 1), "len(vec)71 != shape[0] 70."),
    ("csc", "vmmul", (1, N + 1), "len(vec)71 != shape[0] 70."),
])
def test_shape_refusals(S, layout, call, shape, message):
    ds, D = S.ds[layout], dense(*shape)
    with pytest.raises(ValueError, match=re.escape(message)):
        run(ds, call, D)
    L, out, p = capi.lib(), np.zeros(N * NF), D.ctypes.data_as(C.c_void_p)
    o = out.ctypes.data_as(C.c_void_p)
    rc = {"sd": lambda: L.nfm_dataset_matmul_sd(ds.h, p, shape[0], shape[1], o), "ds": lambda: L.nfm_dataset_matmul_ds(ds.h, p, shape[0], shape[1], o),
          "mvmul": lambda: L.nfm_dataset_mvmul(ds.h, p, shape[0], o), "vmmul": lambda: L.nfm_dataset_vmmul(ds.h, p, shape[1], o)}[call]()
    assert rc == capi.ERR_INVALID and message in L.nfm_last_error().decode()


CHILD = """
import sys, numpy as np, torch
import nimfm_amd as nf
from nimfm_amd import _capi as capi
z = np.load(sys.argv[1])
ds = nf.newCSRDataset(z["data"], z["indices"], z["indptr"], int(z["n"]), int(z["d"]))
D = torch.from_numpy(z["D"]).cuda()
out = torch.full((int(z["n"]), D.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
capi.check(capi.lib().nfm_dataset_matmul_sd_device(ds.h, D.data_ptr(), D.shape[0], D.shape[1], out.data_ptr()))
np.save(sys.argv[2], out.cpu().numpy())
"""


def test_device_form_on_torch_tensors(S, tmp_path):
    """torch goes first in a process of its own, as in bench.py: started after the library it would load a HIP runtime of its own"""
    i, j, v = S.entries["csr"]
    D = dense(NF, 130)
    np.savez(tmp_path / "in.npz", data=v, indices=j, indptr=np.searchsorted(i, np.arange(N + 1)).astype(np.int64), n=N, d=NF, D=D)
    subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npy")], check=True, timeout=300,
                   cwd=ROOT)
    assert np.load(tmp_path / "out.npy").tobytes() == expected(S, "csr", "sd", D).tobytes()
