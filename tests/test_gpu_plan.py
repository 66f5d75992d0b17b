"""-m gpu: the batch plans of all three builders of csrc/plan.hip -- the device-wide sort (uint32 and uint64 keys), the
column-major twin (k_csc_count by table and by key, k_csc_fill<4, 8, 16>) and bucketing (k_seg_* with 32- and 64-bit
items, 4, 8 and 16 items per thread, bucket widths 2^8 .. 2^12, both workgroup orders) -- read back through
nfm_dataset_plan_build / nfm_dataset_plan_get and compared, array for array and scalar for scalar, with the plain
restatement of plan.h in tests/plan_restatement.py.  No tolerance: a plan is integers and copied doubles (tx is compared
as bits).  Which builder and which instantiation built a plan is read back too and asserted per build (`expect` in
tests/plan_cases.py), never assumed; every plan the twin or bucketing built is built again by the sort
(NFM_PLAN_SEG=0 NFM_PLAN_CSC=0) and the two are compared with each other as well.  For every build the route is also
computed from the restatement of csrc/plan_route.h (tests/plan_route_cases.py) and must name what the read-back reports.

The batch >= 2^32 builds rely on plan_build taking a batch longer than the range as the range: before that the twin's
kernels divided by the low 32 bits of the batch (7, or 0) and indexed their histograms with the result.

Not reachable at test size, and not faked: the `cbits < 4` branch of the count-class key (more than 2^28 batches) and
the refusals at T >= 2^31 touches."""
import numpy as np
import pytest

import nimfm_amd as nf
import plan_cases as PC
import plan_route_cases as PR
from gpu_common import _env
from plan_restatement import PLAN_FIELDS, plans_differ, restate

pytestmark = pytest.mark.gpu

PROVENANCE = ("builder", "key_bits", "csc_ne", "csc_by_key", "seg_fl", "seg_nbk", "seg_item_bits", "seg_ipt", "seg_s", "seg_xcd",
              "seg_max_cell")


def read_plan(Xg, build, X, flags, env):
    """One build under exactly the knobs of `env` (every other plan knob unset).  nfm_dataset_plan_get hands back the
    elements the plan defines -- U, TM or T of them -- also where the allocation behind them is rounded up (ucol_s,
    ubeg_s, ucnt_s and hv_u hold at least one element), so whole arrays are compared below."""
    knobs = {k: None for k in PC.KNOBS}
    knobs.update(env)
    begin, end = PC.range_of(build, X)
    kw = dict(begin=begin, end=end, n_aug=build.n_aug, **PC.flags_of(build, flags))
    if build.order[0] == "host":
        kw["perm"] = build.order[1]
    elif build.order[0] == "device":
        kw["device_order"] = build.order[1]
    with _env(**knobs):
        got = Xg.batch_plan(build.batch, **kw)
    route_is_the_restatements(Xg, build, X, flags, env, got)
    return got


ROUTED = ("builder", "csc_ne", "csc_by_key", "seg_fl", "seg_nbk", "seg_item_bits", "seg_ipt", "seg_s", "seg_xcd", "seg_max_cell", "csc_built", "seg_unfit")


def route_is_the_restatements(Xg, build, X, flags, env, got):
    """What the read-back says about who built the plan is what tests/plan_route_cases.py's route() -- the restatement
    tests/test_cpp_plan_route.py holds plan_route.h to -- says for the dataset's shape, the build's arguments and knobs,
    and what the device measured: T, the twin's longest column, the largest cell, and whether the order repeats a sample
    (the twin's clash).  The dataset's state before the build (its twin built, a cell overflowed once) is the read-back of
    the build before on the same dataset."""
    before = getattr(Xg, "_route_state", dict(csc_built=0, seg_unfit=0))
    begin, end = PC.range_of(build, X)
    ns = end - begin
    eff, bp = PR.batch_bounds(ns, build.batch, build.first_singleton)
    assert got["n_batches"] == len(bp) - 1 and got["max_batch"] == max(np.diff(bp), default=0)
    bound_bits = PR.key_bits(X.d, build.n_aug, PR.batch_bound(ns, build.batch))[2]
    assert got["key_bits"] == bound_bits, (got["key_bits"], bound_bits)
    if ns > 0 and got["T"] > 0:
        kind = build.order[0]
        S = PR.Shape(n=X.n, d=X.d, max_row=int(np.diff(X.indptr).max()), n_aug=build.n_aug, begin=begin, end=end, has_order=int(kind != "none"),
                     keyed_order=int(kind == "device"), use_singles=int(bool(flags.get("use_singles"))), first_singleton=int(build.first_singleton),
                     n_batches=len(bp) - 1, max_batch=int(np.diff(bp).max()), has_csc=int(kind != "none"), csc_built=before["csc_built"],
                     max_col=got["csc_max_col"], seg_unfit=before["seg_unfit"])
        clash = int(kind != "none" and len(np.unique(got["perm"])) != ns)
        want = PR.route(S, PR.knobs_of(env), got["T"], clash=clash, h_mx=got["seg_max_cell"])
        assert {k: got[k] for k in ROUTED} == {k: want[k] for k in ROUTED}, (build.tag, flags, env, S, {k: (got[k], want[k]) for k in ROUTED if got[k] != want[k]})
    Xg._route_state = dict(csc_built=got["csc_built"], seg_unfit=got["seg_unfit"])


def describe(p):
    if p["builder"] == "sort":
        return "sort uint%d" % p["key_bits"]
    if p["builder"] == "twin":
        return "twin NE=%d %s" % (p["csc_ne"], "key" if p["csc_by_key"] else "table")
    return "seg fl=%d nbk=%d uint%d ipt=%d cell=%d S=%d xcd=%d" % (p["seg_fl"], p["seg_nbk"], p["seg_item_bits"], p["seg_ipt"],
                                                                  p["seg_max_cell"], p["seg_s"], p["seg_xcd"])


@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_plan_equals_the_restatement(case):
    X = case.data()
    Xg = nf.newCSRDataset(X.data, X.indices, X.indptr, X.n, X.d)
    for build in case.builds:
        begin, end = PC.range_of(build, X)
        for flags in build.flags:
            where = "%s / %s / %s" % (case.name, build.tag, ",".join(k for k, v in sorted(flags.items()) if v) or "-")
            got = read_plan(Xg, build, X, flags, build.env)
            print("PLAN | %s | %s" % (where, describe(got)))
            for k, v in build.expect.items():
                assert got[k] == v, "%s: %s is %r, expected %r (%s)" % (where, k, got[k], v, describe(got))
            if build.order[0] == "device":  # the drawn order: a permutation of the range, then the order of the restatement
                assert np.array_equal(np.sort(got["perm"]), np.arange(begin, end)), where
            perm = PC.resolve_order(build, X, got["perm"])
            want = restate(X.indptr, X.indices, X.data, X.d, build.batch, begin=begin, end=end, perm=perm, n_aug=build.n_aug,
                           **PC.flags_of(build, flags))
            assert plans_differ(got, want) == [], "%s (%s)" % (where, describe(got))
            if build.versus_sort:
                env = dict(build.env, **PC.SORT_ENV)
                by_sort = read_plan(Xg, build, X, flags, env)
                assert by_sort["builder"] == "sort" and by_sort["seg_max_cell"] == 0, where
                assert plans_differ(by_sort, want) == [] and plans_differ(by_sort, got) == [], where


def test_knobs_are_read_per_build():
    """NFM_PLAN_CSC, NFM_PLAN_KEY, NFM_SEG_FL, NFM_SEG_S and NFM_SEG_XCD switched back and forth on one dataset in one
    process: every build follows the value of its moment"""
    case = PC.BY_NAME["twin_device_orders"]
    X = case.data()
    Xg = nf.newCSRDataset(X.data, X.indices, X.indptr, X.n, X.d)
    build = case.builds[-2]
    seen = []
    for env in ({}, {"NFM_PLAN_KEY": "0"}, {"NFM_PLAN_CSC": "0"}, {}, {"NFM_PLAN_KEY": "0"}):
        p = read_plan(Xg, build, X, {}, env)
        seen.append((p["builder"], p["csc_by_key"]))
    assert seen == [("twin", 1), ("twin", 0), ("sort", 0), ("twin", 1), ("twin", 0)]
    case = PC.BY_NAME["seg_batch_counts"]
    X = case.data()
    Xg = nf.newCSRDataset(X.data, X.indices, X.indptr, X.n, X.d)
    seen = []
    for env in ({}, {"NFM_SEG_FL": "8", "NFM_SEG_S": "64", "NFM_SEG_XCD": "0"}, {}, {"NFM_PLAN_SEG": "0"}, {"NFM_SEG_XCD": "0"}):
        p = read_plan(Xg, case.builds[0], X, {}, env)
        seen.append((p["builder"], p["seg_fl"], p["seg_s"], p["seg_xcd"]))
    assert seen == [("seg", 9, 256, 1), ("seg", 8, 64, 0), ("seg", 9, 256, 1), ("sort", 0, 0, 0), ("seg", 9, 256, 0)]


def test_read_back_refuses_what_it_cannot_name():
    X = PC.BY_NAME["sort_exact_counts"].data()
    Xg = nf.newCSRDataset(X.data, X.indices, X.indptr, X.n, X.d)
    with pytest.raises(ValueError):
        Xg.batch_plan(0)
    with pytest.raises(ValueError):
        Xg.batch_plan(4, begin=0, end=X.n + 1)
    with pytest.raises(ValueError):
        Xg.batch_plan(4, perm=np.full(X.n, X.n))
    assert set(PLAN_FIELDS) <= set(Xg.batch_plan(4))
