"""-m gpu.  Which way every mini-batch nfm_opt_epoch call obtained its batch plan.

Results never depend on that way (test_gpu_minibatch.py::test_announced_permutation_is_only_a_hint), so a change that
loses the plan reuse or the plan built beside the previous epoch passes every parity test and only runs slower.  The
library counts the ways, timing enabled or not, under four names of nfm_ctx_timing_get:

  plan_path_built        a plan_build in line for this call
  plan_path_reused       the last plan kept
  plan_path_ahead_taken  the plan built beside the previous epoch (device-drawn or announced order) swapped in
  plan_ahead_built       a next-epoch plan built on the plan stream and marked ready

Every case reads them around each call.  The expected sequences are those of the code before the epoch entry was split
into steps, recorded from that code with only the counters added (DESIGN.md section 19 has the record).

Run as a script (`python tests/test_gpu_plan_paths.py CASE OUT.npz`) the module runs one case and saves the parameters:
the two prefetching cases are held, bit for bit, to the same calls in a child process with NFM_PLAN_PREFETCH=0 (the
variable is read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import nimfm_amd as nf  # noqa: E402
from nimfm_amd import _capi as capi  # noqa: E402
from common import make_perms, random_csr  # noqa: E402
from gpu_common import gpu_fm, to_gpu  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, M, K, B = 3000, 200, 8, 8, 256
PATHS = ("plan_path_built", "plan_path_reused", "plan_path_ahead_taken")
BUILT, REUSED, TAKEN = "built", "reused", "ahead_taken"


def _counters(ctx):
    return [ctx.timing_get(name)[0] for name in PATHS + ("plan_ahead_built",)]


class Run:
    """one optimizer on the shared small problem; call() is one nfm_opt_epoch with the counters read around it"""

    def __init__(self, solver):
        self.Xo = random_csr(N, D, M, seed=17)
        rng = np.random.default_rng(4)
        y = rng.standard_normal(N)
        P0, w0 = rng.standard_normal((1, K, D)) * 0.05, np.zeros(D)
        self.perms = make_perms(N, 4, seed=3)
        self.X = to_gpu(self.Xo)
        self.X.set_targets(y)
        self.ctx = self.X.ctx
        self.fm = gpu_fm("regression", 2, K, "explicit", True, True, P0, w0, 0.0)
        if solver == "mbpsgd":
            self.opt = nf.newMBPSGD(maxIter=1, verbose=0, tol=-1.0, reg=nf.newL1())
            self.opt.batch = B
        else:
            make = nf.newSGD if solver == "sgd" else nf.newAdaGrad
            self.opt = make(maxIter=1, verbose=0, tol=0, mode="minibatch", batch=B)
        self.opt._handle(self.fm, self.ctx, "minibatch")
        self.paths, self.ahead = [], 0

    def announce(self, a, begin=0, end=N):
        capi.check(capi.lib().nfm_opt_announce_perm(self.opt._h, a.ctypes.data, begin, end))

    def set_shuffle(self, seed):
        capi.check(capi.lib().nfm_opt_set_shuffle(self.opt._h, seed))

    def call(self, perm=None, begin=0, end=N):
        before = _counters(self.ctx)
        self.opt._epoch(self.X, perm, begin, end)
        delta = [a - b for a, b in zip(_counters(self.ctx), before)]
        assert sorted(delta[:3]) == [0, 0, 1], "one call takes exactly one of the three ways: %r" % (delta,)
        self.paths.append((BUILT, REUSED, TAKEN)[delta[:3].index(1)])
        self.ahead += delta[3]

    def params(self):
        self.opt._finalize_into(self.fm)
        return np.array(self.fm.P), np.array(self.fm.w), np.float64(self.fm.intercept)


def case_sgd_same_range():
    r = Run("sgd")
    for _ in range(3):
        r.call()
    return r


def case_adagrad_same_range():
    r = Run("adagrad")  # (it = 1: the first step is a mini-batch of its own, so the key changes once)
    for _ in range(3):
        r.call()
    return r


def case_sgd_announce():
    """the calls of test_announced_permutation_is_only_a_hint"""
    r = Run("sgd")
    p = r.perms
    decoy = np.ascontiguousarray(p[3][::-1])
    r.announce(p[1])
    r.call(p[0])        # the plan of p[1] is built beside this epoch
    r.call(p[1])        # ... and taken
    r.announce(decoy)
    r.call(p[2])        # (the decoy's plan is built beside it and never asked for)
    changed = p[3].copy()
    r.announce(changed)
    r.call(p[2])
    changed[[0, -1]] = changed[[-1, 0]]  # the promised array was modified at both ends: the probes notice
    r.call(changed)
    r.keep = (decoy, changed)  # (announced arrays stay alive as long as the optimizer may look at them)
    return r


def case_sgd_shuffle():
    r = Run("sgd")
    r.set_shuffle(7)
    for _ in range(3):
        r.call()
    return r


def case_adagrad_shuffle():
    r = Run("adagrad")  # (the plan ahead is built with first_singleton = false: what call 2 needs)
    r.set_shuffle(7)
    for _ in range(3):
        r.call()
    return r


def case_sgd_shuffle_timed():
    r = Run("sgd")
    r.set_shuffle(7)
    r.ctx.timing_enable(True)
    try:
        for _ in range(3):
            r.call()
    finally:
        r.ctx.timing_enable(False)
    return r


def case_sgd_other_range():
    r = Run("sgd")
    r.call(None, 0, N)
    r.call(None, 0, 2000)
    r.call(None, 0, N)
    return r


def case_mbpsgd_announce():
    r = Run("mbpsgd")
    end = N // B * B  # (MBPSGD takes whole mini-batches)
    r.announce(r.perms[1], 0, end)
    r.call(r.perms[0], 0, end)
    r.call(r.perms[1], 0, end)  # the announcement is ignored for it
    return r


CASES = {
    "sgd_same_range": (case_sgd_same_range, [BUILT, REUSED, REUSED], 0),
    "adagrad_same_range": (case_adagrad_same_range, [BUILT, BUILT, REUSED], 0),
    "sgd_announce": (case_sgd_announce, [BUILT, TAKEN, BUILT, BUILT, BUILT], 3),
    "sgd_shuffle": (case_sgd_shuffle, [BUILT, TAKEN, TAKEN], 3),
    "adagrad_shuffle": (case_adagrad_shuffle, [BUILT, TAKEN, TAKEN], 3),
    "sgd_shuffle_timed": (case_sgd_shuffle_timed, [BUILT, BUILT, BUILT], 0),
    "sgd_other_range": (case_sgd_other_range, [BUILT, BUILT, BUILT], 0),
    "mbpsgd_announce": (case_mbpsgd_announce, [BUILT, BUILT], 0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_plan_path_of_every_call(case, tmp_path):
    assert os.environ.get("NFM_PLAN_PREFETCH") is None, "the expected sequences are those of the default setting"
    run, paths, ahead = CASES[case]
    r = run()
    print("plan paths %s: %s, plan_ahead_built %d" % (case, ", ".join(r.paths), r.ahead))
    assert r.paths == paths
    assert r.ahead == ahead
    if case in ("sgd_announce", "sgd_shuffle"):
        # a hint only: the same calls with every plan built in line give the same bits
        out = str(tmp_path / "inline.npz")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), case, out], cwd=ROOT, env=dict(os.environ, NFM_PLAN_PREFETCH="0"),
                               capture_output=True, text=True, timeout=300)
        assert child.returncode == 0, (child.stdout[-2000:], child.stderr[-2000:])
        assert "plan_ahead_built 0" in child.stdout, child.stdout[-500:]
        want = np.load(out)
        for got, name in zip(r.params(), ("P", "w", "b")):
            assert np.array_equal(got, want[name]), name + " differs from the run with NFM_PLAN_PREFETCH=0"


if __name__ == "__main__":
    r = CASES[sys.argv[1]][0]()
    print("plan paths %s: %s, plan_ahead_built %d" % (sys.argv[1], ", ".join(r.paths), r.ahead))
    P, w, b = r.params()
    np.savez(sys.argv[2], P=P, w=w, b=b)
