"""CPU: tests/plan_restatement.py is the definition tests/test_gpu_plan.py holds the library's batch plans to, and
tests/plan_cases.py the inputs.  Here, without a GPU: the restatement equals a brute-force builder (dictionaries and
loops) on tiny inputs; every case has the property its name claims, computed from the data alone; every plan the cases
expect from bucketing or from the column-major twin meets that builder's conditions as plan.hip's comments state them, so
that an `expect` is a statement about the data and not a guess; and the cases tell the definition from its neighbours."""
import numpy as np
import pytest

import plan_cases as PC
from plan_restatement import batch_bounds, plans_differ, restate


# ---------------------------------------------------------------- brute force
def brute(X, batch, begin, end, perm, n_aug, first_singleton, want_tq, use_singles, sort_by_count):
    ns = end - begin
    bounds = [0] + ([1] if first_singleton and ns > 0 else [])
    while bounds[-1] < ns:
        bounds.append(min(bounds[-1] + min(batch, ns), ns))
    groups, toff, t = {}, [0], 0
    for p in range(ns):
        i = perm[begin + p] if perm is not None else begin + p
        b = max(k for k in range(len(bounds) - 1) if bounds[k] <= p)
        row = [(int(X.indices[e]), X.data[e]) for e in range(X.indptr[i], X.indptr[i + 1])] + [(X.d + a, 1.0) for a in range(n_aug)]
        for j, x in row:
            groups.setdefault((b, j), []).append((p - bounds[b], x, t))
            t += 1
        toff.append(t)
    single = [0] * t
    out = dict(ucol=[], uptr=[0], tpos=[], tx=[], tq=[], ub=[], hv_u=[], hv_seg0=[0])
    for (b, j) in sorted(groups):
        g = groups[(b, j)]
        if use_singles and len(g) == 1:
            single[g[0][2]] = 1
            continue
        if len(g) > 128:
            out["hv_u"].append(len(out["ucol"]))
            out["hv_seg0"].append(out["hv_seg0"][-1] + (len(g) + 63) // 64)
        out["ucol"].append(j)
        out["ub"].append(b)
        for pib, x, tt in g:
            out["tpos"].append(pib), out["tx"].append(x), out["tq"].append(tt)
        out["uptr"].append(len(out["tpos"]))
    U = len(out["ucol"])
    cnt = [out["uptr"][u + 1] - out["uptr"][u] for u in range(U)]
    order = sorted(range(U), key=lambda u: (out["ub"][u], -min(cnt[u], 15), out["ucol"][u])) if sort_by_count else list(range(U))
    out.update(ucol_s=[out["ucol"][u] for u in order], ubeg_s=[out["uptr"][u] for u in order], ucnt_s=[cnt[u] for u in order])
    nb = len(bounds) - 1
    out["bat_pos"] = bounds
    out["bat_uoff"] = [sum(1 for x in out["ub"] if x < b) for b in range(nb + 1)]
    out["bat_toff"] = [out["uptr"][u] for u in out["bat_uoff"]]
    out["bat_hoff"] = [sum(1 for h in out["hv_u"] if h < u) for u in out["bat_uoff"]]
    out["bat_soff"] = [out["hv_seg0"][h] for h in out["bat_hoff"]]
    out["single"], out["toff"] = single, toff
    return out


def _tiny(seed, n, d, max_m):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_m + 1, size=n)
    return PC.strided_rows(lens, d, seed + 100, unsorted=True)


TINY = [
    # data,                 batch, begin, end, order,  n_aug, first_singleton
    (_tiny(1, 23, 7, 5), 4, 0, 23, None, 0, False),
    (_tiny(2, 23, 7, 5), 4, 3, 20, "perm", 0, False),
    (_tiny(3, 30, 5, 4), 7, 0, 30, "perm", 2, True),
    (_tiny(4, 30, 9, 3), 30, 2, 29, None, 1, True),
    (_tiny(5, 12, 6, 6), 5, 0, 40, "stream", 0, False),
    (_tiny(6, 300, 4, 3), 140, 0, 300, "perm", 1, False),  # features of more than 128 touches: heavy
    (_tiny(7, 9, 6, 4), 100, 0, 9, None, 0, True),          # a batch longer than the range
]


@pytest.mark.parametrize("idx", range(len(TINY)))
@pytest.mark.parametrize("flags", PC.ALL8, ids=lambda f: "".join("1" if f[k] else "0" for k in ("want_tq", "use_singles", "sort_by_count")))
def test_restatement_equals_brute_force(idx, flags):
    X, batch, begin, end, order, n_aug, fs = TINY[idx]
    rng = np.random.default_rng(50 + idx)
    perm = {None: None, "perm": rng.permutation(X.n), "stream": rng.integers(0, X.n, size=end)}[order]
    R = restate(X.indptr, X.indices, X.data, X.d, batch, begin, end, perm, n_aug, fs, **flags)
    B = brute(X, batch, begin, end, perm, n_aug, fs, **flags)
    assert R["T"] > 0
    names = ["bat_pos", "ucol", "uptr", "tpos", "ucol_s", "ubeg_s", "ucnt_s", "bat_uoff", "bat_toff", "bat_hoff", "bat_soff", "hv_u"]
    names += ["tq"] if flags["want_tq"] else []
    names += ["single"] if flags["use_singles"] else []
    names += ["toff"] if flags["want_tq"] or flags["use_singles"] else []
    for k in names:
        assert list(R[k]) == list(B[k]), k
    assert [float(x) for x in R["tx"]] == [float(x) for x in B["tx"]]
    assert list(R["hv_seg0"]) == (B["hv_seg0"] if B["hv_u"] else [])
    assert (R["U"], R["TM"], R["H"], R["HS"]) == (len(B["ucol"]), len(B["tpos"]), len(B["hv_u"]), B["hv_seg0"][-1])
    assert R["max_unique"] == max(np.diff(B["bat_uoff"])) and R["max_heavy"] == max(np.diff(B["bat_hoff"]))
    assert R["max_segs"] == max(np.diff(B["bat_soff"])) and R["max_batch"] == max(np.diff(B["bat_pos"]))
    if idx == 5:
        assert R["H"] > 0


def test_batch_bounds():
    assert list(batch_bounds(0, 4, False)) == [0] and list(batch_bounds(0, 4, True)) == [0]
    assert list(batch_bounds(1, 4, True)) == [0, 1] and list(batch_bounds(9, 4, True)) == [0, 1, 5, 9]
    assert list(batch_bounds(9, 4, False)) == [0, 4, 8, 9] and list(batch_bounds(8, 4, False)) == [0, 4, 8]
    assert list(batch_bounds(9, 2**32 + 7, False)) == [0, 9] and list(batch_bounds(9, 2**63 - 1, True)) == [0, 1, 9]


# ---------------------------------------------------------------- the construction claims
def _builds():
    return [(c, b) for c in PC.CASES for b in c.builds]


def _ids():
    return ["%s/%s" % (c.name, b.tag) for c, b in _builds()]


def _cpu_order(build, data):
    """the order as far as it is known without a device: a drawn order is some permutation of its range, and every claim
    made for such a build is about the SET of samples in the range (tests/test_gpu_plan.py checks the read-back is one)"""
    if build.order[0] == "device":
        return np.arange(PC.range_of(build, data)[1], dtype=np.int64)
    return PC.resolve_order(build, data)


def _ipt_of(cell):
    return 4 if cell <= 1024 else 8 if cell <= 2048 else 16


def _ne_of(col):
    return 4 if col <= 256 else 8 if col <= 512 else 16


@pytest.mark.parametrize("case,build", _builds(), ids=_ids())
def test_case_has_the_property_its_name_claims(case, build):
    X = case.data()
    perm = _cpu_order(build, X)
    begin, end = PC.range_of(build, X)
    assert 0 <= begin <= end and (end <= X.n or perm is not None) and (perm is None or len(perm) >= end)
    b, f, bp, m = PC.touch_table(X, build, perm)
    nb, T = len(bp) - 1, int(m.sum()) + build.n_aug * (end - begin)
    col_len = np.bincount(X.indices, minlength=X.d) if len(X.indices) else np.zeros(X.d, dtype=np.int64)
    ex, cl = build.expect, dict(build.claims)
    if "n_batches" in ex:
        assert nb == ex["n_batches"]
    repeats = perm is not None and len(np.unique(perm[begin:end])) < end - begin
    dense = nb > 0 and T >= 0.5 * nb * X.d
    twin_may = (perm is not None and build.n_aug == 0 and end <= X.n and nb <= 512 and nb * X.d <= 2**28 and dense
                and not build.env.get("NFM_PLAN_CSC") == "0")
    # -- what a build expected from the twin must be: an order without repeats, dense, few batches, short columns
    if ex.get("builder") == "twin":
        assert twin_may and not repeats and all(not fl.get("use_singles") for fl in build.flags)
        assert col_len.max() <= 1024 and ex["csc_ne"] == _ne_of(col_len.max())
        assert ex["csc_by_key"] == (1 if build.order[0] == "device" and build.env.get("NFM_PLAN_KEY") != "0" else 0)
    # -- and from bucketing: not the twin's, 8192 touches per batch, cells that fit
    if ex.get("builder") == "seg":
        assert not twin_may and build.n_aug == 0 and build.env.get("NFM_PLAN_SEG") != "0"
        fl = ex["seg_fl"]
        assert fl == (int(build.env["NFM_SEG_FL"]) if "NFM_SEG_FL" in build.env else PC.natural_fl(X, build, perm))
        nbk = ((X.d - 1) >> fl) + 1
        cell = PC.largest_cell(X, build, perm, fl)
        assert nbk <= 4096 and T / nb / nbk <= 3072 and cell <= 4096 and ex["seg_ipt"] == _ipt_of(cell)
        assert ex.get("seg_nbk", nbk) == nbk and ex.get("seg_max_cell", cell) == cell
        assert ex["seg_item_bits"] == (32 if PC.item_bit_sum(X, build, fl) <= 32 else 64)
    if ex.get("builder") == "sort" and build.env.get("NFM_PLAN_SEG") != "0":
        # left to the sort with every knob at its default: the claims below say why
        assert cl.keys() & {"max_col", "repeats", "max_cell", "touches_per_batch_at_least"} or nb > 512 or T / max(nb, 1) < 8192
    # -- the named claims
    if "touches_per_batch_at_least" in cl:
        assert T / nb >= cl.pop("touches_per_batch_at_least")
    if "item_sum_fits" in cl:
        assert PC.item_bit_sum(X, build, cl.pop("item_sum_fits")) <= 32
    if "item_sum_over" in cl:
        assert PC.item_bit_sum(X, build, cl.pop("item_sum_over")) > 32
    if "item_sum" in cl:
        assert PC.item_bit_sum(X, build, ex["seg_fl"]) == cl.pop("item_sum")
    if "natural_fl" in cl:
        assert PC.natural_fl(X, build, perm) == cl.pop("natural_fl")
    if "max_cell" in cl:
        fl, M = cl.pop("max_cell")
        assert PC.largest_cell(X, build, perm, fl) == M
    if "max_row" in cl:
        assert np.diff(X.indptr).max() == cl.pop("max_row")
    if "max_batch" in cl:
        assert np.diff(bp).max() == cl.pop("max_batch")
    if "d_ragged" in cl:
        assert X.d % (1 << cl.pop("d_ragged")) != 0
    if "key_sum" in cl:
        assert PC.key_bit_sum(X, build) == cl.pop("key_sum")
    if "max_col" in cl:
        assert col_len.max() == cl.pop("max_col")
    if "max_col_in" in cl:
        lo, hi = cl.pop("max_col_in")
        assert lo <= col_len.max() <= hi
    if "empty_columns" in cl:
        assert all(col_len[j] == 0 for j in cl.pop("empty_columns")) and X.d % 4 != 0
    if "unsorted" in cl:
        cl.pop("unsorted")
        rows = np.repeat(np.arange(X.n), np.diff(X.indptr))
        assert ((rows[1:] == rows[:-1]) & (X.indices[1:] < X.indices[:-1])).any()
    if "columns_outside" in cl:
        out = cl.pop("columns_outside")
        inside = np.bincount(f, minlength=X.d)
        assert all(inside[j] == 0 and col_len[j] > 0 for j in out)
        assert any(0 < inside[j] < col_len[j] for j in range(X.d))
    if "repeats" in cl:
        cl.pop("repeats")
        assert repeats and twin_may
    if "dense" in cl:
        cl.pop("dense")
        assert dense
    if "cells_above" in cl:
        assert nb * X.d > cl.pop("cells_above")
    counts = np.unique(b * np.int64(X.d) + f, return_counts=True)[1] if len(f) else np.zeros(0, dtype=np.int64)
    if "counts" in cl:
        assert sorted(counts) == cl.pop("counts")
    if "counts_max" in cl:
        assert counts.max() == cl.pop("counts_max")
    if "dummy_touches" in cl:
        assert build.n_aug >= 1 and np.diff(bp).min() == cl.pop("dummy_touches") > 128
    if "empty_batches" in cl:
        assert sorted(set(range(nb)) - set(b.tolist())) == cl.pop("empty_batches")
    if "single_only_batch" in cl:
        bb = cl.pop("single_only_batch")
        key = b * np.int64(X.d) + f
        u, c = np.unique(key, return_counts=True)
        assert (c[u // X.d == bb] == 1).all() and (u // X.d == bb).any() and (c[u // X.d != bb] > 1).any()
    if "heavy_batches" in cl:
        key = b * np.int64(X.d) + f
        u, c = np.unique(key, return_counts=True)
        assert sorted(set((u[c > 128] // X.d).tolist())) == cl.pop("heavy_batches")
    if "single_cell" in cl:
        k, fl = cl.pop("single_cell"), ex["seg_fl"]
        key = b * np.int64(X.d) + f
        u, c = np.unique(key, return_counts=True)
        in_cell = (u % X.d) >> fl == k
        assert in_cell.sum() > 1000 and (c[in_cell] == 1).all() and (c[~in_cell] > 1).any()
    assert not cl, "claims nobody checked: %s" % sorted(cl)


def test_the_edges_the_issue_names_are_all_placed():
    ex = [(c.name, b, b.expect) for c in PC.CASES for b in c.builds]
    twin = [e for _, _, e in ex if e.get("builder") == "twin"]
    seg = [(b, e) for _, b, e in ex if e.get("builder") == "seg"]
    assert {e["csc_ne"] for e in twin} == {4, 8, 16} and {e["csc_by_key"] for e in twin} == {0, 1}
    assert {e["seg_ipt"] for _, e in seg} == {4, 8, 16} and {e["seg_item_bits"] for _, e in seg} == {32, 64}
    assert {e["seg_fl"] for b, e in seg if "NFM_SEG_FL" not in b.env} == {8, 9, 10, 11, 12}
    assert {e["seg_fl"] for b, e in seg if "NFM_SEG_FL" in b.env} == {8, 9, 11, 12}
    assert {e.get("seg_max_cell") for _, _, e in ex} >= {1024, 1025, 2048, 2049, 4096, 4097}
    assert {e.get("key_bits") for _, _, e in ex} >= {32, 64}
    assert {e.get("n_batches") for _, b, e in ex if e.get("builder") == "seg"} >= {1, 7, 8, 9}
    assert {e.get("n_batches") for _, b, e in ex if e.get("builder") == "twin"} >= {1, 64, 65, 512}
    assert 2**32 + 7 in {b.batch for _, b, e in ex if e.get("builder") == "twin"} and 2**32 in {b.batch for _, b, _ in ex}


# ---------------------------------------------------------------- the cases discriminate
MUTATIONS = {
    "heavy threshold 127": dict(heavy_above=127),
    "heavy threshold 129": dict(heavy_above=129),
    "segment length 63": dict(segment=63),
    "class clamp 14": dict(class_clamp=14),
    "class clamp 16": dict(class_clamp=16),
    "touches by descending position": dict(descending_positions=True),
    "singles threshold off by one": dict(single_max=2),
    "dummy features before the row's entries": dict(dummies_first=True),
}
SMALL = ("sort_ragged", "sort_exact_counts", "sort_heavy_edges", "sort_dummies_heavy", "sort_all_singles_batch")


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_cases_tell_the_definition_from_its_neighbours(name):
    caught = []
    for cname in SMALL:
        case = PC.BY_NAME[cname]
        X = case.data()
        for build in case.builds:
            if build.order[0] == "device":
                continue
            begin, end = PC.range_of(build, X)
            for fl in build.flags:
                kw = dict(begin=begin, end=end, perm=PC.resolve_order(build, X), n_aug=build.n_aug, **PC.flags_of(build, fl))
                true = restate(X.indptr, X.indices, X.data, X.d, build.batch, **kw)
                wrong = restate(X.indptr, X.indices, X.data, X.d, build.batch, **kw, **MUTATIONS[name])
                if plans_differ(true, wrong):
                    caught.append((cname, build.tag))
    assert caught, "no case tells the definition from: %s" % name
