"""The inputs of the crossDecisionFunction / recommend tests (tests/test_cross_restatement.py on the CPU, tests/test_gpu_cross.py
on the device).  A case is U, V (lists of rows of (column id, value) in storage order), their widths, P [k][dU + dV + nAug], w, b,
lams, K and the model's options.  Rows are empty, one entry long, unsorted, or repeat an id; `tie` names two identical rows of V, the best item of the last user and a copy
of it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_shape():
    """The tile of crossDecisionFunction / recommend as nimfm_amd/csrc/cross.h states it: {"TU": users, "TV": items, "KS": the
    factor loop's step, "maxTopK"} -- read from the header, so that the tests of the tile's edges type no number of their own."""
    text = open(os.path.join(ROOT, "nimfm_amd", "csrc", "cross.h")).read()
    names = {"TU": "kCrossTU", "TV": "kCrossTV", "KS": "kCrossKS", "maxTopK": "kCrossMaxTopK"}
    return {k: int(re.search(r"constexpr int %s = (\d+);" % v, text).group(1)) for k, v in names.items()}


def make_rows(rng, n, d, mean_len):
    rows = []
    for i in range(n):
        m = int(rng.randint(0, 2 * mean_len + 1))
        ids = [int(j) for j in rng.randint(0, d, size=m)] if d else []
        if i % 3 == 0:
            ids = sorted(set(ids))  # ascending and distinct, as a loader leaves them
        rows.append([(j, float(rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0]))) for j in ids])
    if n > 1:
        rows[0] = []  # an empty row
        rows[1] = [(d - 1, 0.75)]  # one entry
    if n > 2 and d > 2:
        rows[2] = [(2, 1.25), (0, -0.5), (2, 0.625), (1, 1.0)]  # unsorted, with a repeated id
    return rows


def n_aug(fitLower, fitLinear, degree=2):
    """model/factorization_machine.nim:81-86"""
    return (degree - 2 if fitLinear else degree - 1) if fitLower == "augment" else 0


def make_case(name, seed, nU, nV, dU, dV, k, K, fitLower="explicit", fitLinear=True, fitIntercept=True, tie=None, lams=False, mean_len=4):
    rng = np.random.RandomState(seed)
    na = n_aug(fitLower, fitLinear)
    U, V = make_rows(rng, nU, dU, mean_len), make_rows(rng, nV, dV, mean_len)
    case = {
        "name": name, "U": U, "V": V, "dU": dU, "dV": dV, "k": k, "K": K, "nAug": na, "tie": tie,
        "fitLower": fitLower, "fitLinear": fitLinear, "fitIntercept": fitIntercept,
        "P": rng.normal(0.0, 0.4, size=(k, dU + dV + na)),
        "w": rng.normal(0.0, 1.0, size=dU + dV) if fitLinear else np.zeros(dU + dV),
        "b": float(rng.normal()) if fitIntercept else 0.0,
        "lams": rng.uniform(0.5, 1.5, size=k) if lams else np.ones(k),
    }
    if tie:  # the last user's best item, copied over another one: the tie is inside a top K
        import cross_restatement as R
        best = R.rank(R.cross(dict(case, U=U[-1:]))[0], 1)[0][0]
        other = tie if tie != best else tie + 1
        V[other] = list(V[best])
        case["tie"] = (min(best, other), max(best, other))
    return case


def cases():
    return [
        make_case("explicit", 11, nU=5, nV=70, dU=6, dV=9, k=3, K=7),
        make_case("none_no_linear", 12, nU=33, nV=9, dU=12, dV=5, k=65, K=2, fitLower="none", fitLinear=False),
        make_case("augment_dummy_tie", 13, nU=4, nV=130, dU=7, dV=11, k=8, K=10, fitLower="augment", fitLinear=False, fitIntercept=False, tie=77),
        make_case("augment_linear_all", 14, nU=3, nV=3, dU=3, dV=4, k=1, K=3, fitLower="augment"),
        make_case("wide_lams", 15, nU=3, nV=20, dU=9, dV=8, k=129, K=1, lams=True),
    ]


def csr_arrays(rows):
    """-> (data, indices, indptr) for newCSRDataset"""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, r in enumerate(rows):
        indptr[i + 1] = indptr[i] + len(r)
    indices = np.array([j for r in rows for j, _ in r], dtype=np.int64)
    data = np.array([x for r in rows for _, x in r], dtype=np.float64)
    return data, indices, indptr
