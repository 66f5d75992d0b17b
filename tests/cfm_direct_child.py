"""One Hazan fit of the `cg_long` input and one GreedyCD fit of a grid case of tests/cfm_grid_cases.py on the device, for
test_launch_by_launch_equals_the_graph of tests/test_gpu_cfm_grid.py.  cfm.hip reads NFM_HAZAN_GRAPH once per process, so the
run without the captured chunks needs a process of its own: the test calls compare(), which runs fits() here (the captured
graphs) and in a child started with NFM_HAZAN_GRAPH=0 (every launch issued one by one), and holds the two bit-equal.

    python tests/cfm_direct_child.py OUT.npz"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _flat(history):
    """every number of a history (a list of records, GreedyCD's with a list of inner records), in a fixed order"""
    out = []
    for r in history:
        for key in sorted(r):
            if key == "inner":
                out += [float(x[k]) for x in r[key] for k in sorted(x)]
            else:
                out.append(float(r[key]))
    return np.array(out)


def fits():
    """-> the arrays of both fits: the CG of more than one chunk, and the power method ending one past a chunk"""
    import nimfm_amd as nf

    import cfm_grid_cases as G
    import test_gpu_cfm_grid as T
    out = {}
    cfm, opt = T.hazan_device_fit(nf, *G.CG_LONG_RUN)
    out.update(hP=cfm.P, hlams=cfm.lams, hw=cfm.w, hb=np.float64(cfm.intercept), hhist=_flat(opt.history),
               hcg=np.array([r["cgIters"] for r in opt.history]))
    cfm, opt = T.gcd_device_fit(nf, G.GCD_GRID_CASE)
    out.update(gP=cfm.P, glams=cfm.lams, gw=cfm.w, gb=np.float64(cfm.intercept), ghist=_flat(opt.history))
    return out


def compare(tmp_path, chunk):
    out = os.path.join(str(tmp_path), "direct.npz")
    env = dict(os.environ, NFM_HAZAN_GRAPH="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    direct = np.load(out)
    assert str(direct["graph_env"]) == "0"
    here = fits()
    assert os.environ.get("NFM_HAZAN_GRAPH", "1") != "0"  # this process replays the captured chunks
    assert here["hcg"][0] > chunk and np.isfinite(here["hhist"]).all() and np.isfinite(here["ghist"]).all()
    for key, val in here.items():
        assert np.array_equal(direct[key], val), key


if __name__ == "__main__":
    res = fits()
    np.savez(sys.argv[1], graph_env=os.environ.get("NFM_HAZAN_GRAPH", ""), **res)
