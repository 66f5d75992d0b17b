"""One PBCD fit with OmegaCS of the `edges` case of tests/cd_schedule_cases.py on the device, for
tests/test_gpu_pbcd_omegacs.py::test_direct_launches_equal_the_graph.  cd.hip reads NFM_CD_GRAPH once per process, so the run
without the captured graph needs a process of its own, as in tests/cd_direct_child.py: compare() runs fit_edges() here (the
captured graph) and in a child started with NFM_CD_GRAPH=0, and holds the two bit-equal.

    python tests/pbcd_omegacs_direct_child.py DEGREE OUT.npz"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def fit_edges(degree):
    """-> (P, w, intercept, history) after 3 iterations with intercept, linear term and explicit lower orders"""
    import cd_schedule_cases as S
    import test_gpu_pbcd_omegacs as T
    Xo, y = S.inputs("edges")
    P0, w0, b0, _ = S.start(Xo, degree, 4, "explicit", True, True)
    fm, opt = T.device_fit(T.csr_of(Xo), y, P0, w0, b0, degree, "explicit", True, True, maxIter=3, tol=0.0,
                           gamma=T.GAMMA["edges", degree, 4, "explicit"])
    return fm.P, fm.w, np.float64(fm.intercept), np.array(opt.history)


def compare(degree, tmp_path):
    out = os.path.join(str(tmp_path), "direct.npz")
    env = dict(os.environ, NFM_CD_GRAPH="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(degree), out], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    direct = np.load(out)
    assert str(direct["graph_env"]) == "0"
    P, w, b, hist = fit_edges(degree)
    assert os.environ.get("NFM_CD_GRAPH", "1") != "0"  # this process replays the captured graph
    assert hist.shape == (3, 2) and np.isfinite(hist).all()
    assert np.array_equal(direct["P"], P) and np.array_equal(direct["w"], w) and direct["b"] == b
    assert np.array_equal(direct["hist"], hist)


if __name__ == "__main__":
    degree, out = sys.argv[1:3]
    P, w, b, hist = fit_edges(int(degree))
    np.savez(out, P=P, w=w, b=b, hist=hist, graph_env=os.environ.get("NFM_CD_GRAPH", ""))
