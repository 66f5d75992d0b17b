"""-m gpu: `python -m nimfm_amd train --solver katyusha` (the reference's nimfm_sparsefm train, src/nimfm_sparsefm.nim:64-68) end
to end: ingest, fit, dump, then `test` on the dump -- and the dump equals a Python fit with the same options, value for
value (with --shuffle false both consume the identity stream with wrap-around)."""
import numpy as np
import pytest

import nimfm_amd as nf
from test_gpu_pcd import _cli, _files

pytestmark = pytest.mark.gpu
REGS = {"l1": nf.newL1, "l21": nf.newL21, "squaredl12": nf.newSquaredL12, "squaredl21": nf.newSquaredL21}


@pytest.mark.parametrize("reg,extra", [("squaredl12", {}), ("l1", {"miniBatchSize": 16, "eta0": 0.05})])
def test_dump_equals_a_python_fit(tmp_path, reg, extra):
    train = _files(tmp_path)
    dump = str(tmp_path / "fm.txt")
    args = ["train", "--task", "r", "--train", train, "--solver", "katyusha", "--reg", reg, "--gamma", "1e-3", "--maxIter", "3",
            "--nComponents", "3", "--verbose", "0", "--shuffle", "false", "--dump", dump]
    for k, v in extra.items():
        args += ["--" + k, str(v)]
    r = _cli(args)
    assert r.returncode == 0, r.stderr
    got = nf.load(dump, False)
    X, y = nf.loadSVMLightFile(train, -1)
    fm = nf.newFactorizationMachine("regression", degree=2, nComponents=3, randomState=1, scale=0.1)
    kw = dict(maxIter=3, eta=extra.get("eta0", 0.1), alpha0=1e-7, alpha=1e-5, beta=1e-3, gamma=1e-3, reg=REGS[reg](),
              miniBatchSize=extra.get("miniBatchSize", -1), verbose=0, tol=1e-5, shuffle=False, lossParam=0.1)
    nf.newKatyusha(**kw).fit(X, y, fm)
    ref = str(tmp_path / "ref.txt")
    fm.dump(ref)
    want = nf.load(ref, False)  # through the same text format: the dump's digits are what is compared
    assert np.array_equal(got.P, want.P) and np.array_equal(got.w, want.w) and got.intercept == want.intercept
    assert np.isfinite(got.P).all()
    r = _cli(["test", "--task", "r", "--test", train, "--load", dump])  # `test` reads the dump back
    assert r.returncode == 0 and "Test RMSE" in r.stdout, r.stderr


def test_verbose_and_refusals(tmp_path):
    train = _files(tmp_path)
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "katyusha", "--maxIter", "2", "--verbose", "1", "--nComponents", "3"])
    assert r.returncode == 0, r.stderr
    assert "Minibatch size" in r.stdout and "Violation" in r.stdout and "Objective did not converge" in r.stdout
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "katyusha", "--reg", "omegati"])
    assert r.returncode != 0 and "regularization omegati is not supported" in r.stderr
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "katyusha", "--reg", "squaredl12", "--degree", "3", "--nComponents", "3"])
    assert r.returncode != 0 and "SquaredL12 supports only degree=2." in r.stderr
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "katyusha", "--beta", "0"])
    assert r.returncode != 0 and "beta must be > 0" in r.stderr
    r = _cli(["train", "--task", "r", "--train", train, "--solver", "cd"])  # still refused, with its own message
    assert r.returncode != 0 and "not supported" in r.stderr
