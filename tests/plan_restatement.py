"""The batch plan (nimfm_amd/csrc/plan.h) restated in vectorised numpy, in the header's words.  It shares nothing with
plan.hip: no keys, no buckets, no column-major copy -- one stable sort of the touches by (batch, feature) and counting.

restate(...) returns a dict with every field of `Plan` that nfm_dataset_plan_get hands back.  The keyword arguments after
`sort_by_count` are the definition's constants; tests/test_plan_restatement.py changes one at a time to show that the
cases of tests/plan_cases.py tell the true definition from its neighbours.

Two things the library's build leaves unmade are restated as the library leaves them, not as plan.h would suggest:
an empty range (end == begin) returns before bat_hoff / bat_soff exist, and a range without a single touch (T == 0)
returns with uptr = [0] and nothing else: no toff, no single, no bat_hoff / bat_soff."""
import numpy as np

I64 = np.int64


def batch_bounds(ns, batch, first_singleton):
    """bat_pos: start at 0, one sample first under first_singleton, then steps of `batch`; a batch longer than the range
    is the range"""
    eff = min(int(batch), max(int(ns), 1))
    start = 1 if (first_singleton and ns > 0) else 0
    pts = list(range(start, ns, eff)) + [ns]
    return np.array(([0] if start == 1 else []) + pts, dtype=I64)


def restate(indptr, indices, data, d, batch, begin=0, end=None, perm=None, n_aug=0, first_singleton=False, want_tq=False,
            use_singles=False, sort_by_count=False, heavy_above=128, segment=64, class_clamp=15, single_max=1,
            descending_positions=False, dummies_first=False):
    indptr, indices, data = np.asarray(indptr, dtype=I64), np.asarray(indices, dtype=I64), np.asarray(data, dtype=np.float64)
    n = len(indptr) - 1
    end = n if end is None else int(end)
    ns = end - begin
    P = {}
    bat_pos = batch_bounds(ns, batch, first_singleton)
    nb = len(bat_pos) - 1
    P["bat_pos"], P["n_batches"], P["batch"] = bat_pos, nb, int(batch)
    P["max_batch"] = int(np.diff(bat_pos).max()) if nb else 0
    empty = dict(perm=("<i8", 0), ucol=("<i4", 0), uptr=("<i8", 0), ucol_s=("<i4", 0), ubeg_s=("<i8", 0), ucnt_s=("<i4", 0),
                 tpos=("<i4", 0), tx=("<f8", 0), tq=("<i8", 0), toff=("<i8", 0), single=("u1", 0), hv_u=("<i8", 0),
                 hv_seg0=("<i8", 0))
    for k, (dt, _) in empty.items():
        P[k] = np.zeros(0, dtype=dt)
    for k in ("U", "T", "TM", "max_unique", "H", "HS", "max_heavy", "max_segs"):
        P[k] = 0
    P["bat_uoff"] = np.zeros(nb + 1, dtype=I64)
    P["bat_toff"] = np.zeros(nb + 1, dtype=I64)
    P["bat_hoff"] = np.zeros(0, dtype=I64)
    P["bat_soff"] = np.zeros(0, dtype=I64)
    if ns == 0:
        return P
    # the sample at a position
    pos = np.arange(ns, dtype=I64)
    samp = np.asarray(perm, dtype=I64)[begin:end] if perm is not None else begin + pos
    if perm is not None:
        P["perm"] = samp.copy()
    m = indptr[samp + 1] - indptr[samp]
    toff = np.concatenate([[0], np.cumsum(m + n_aug)]).astype(I64)
    T = int(toff[-1])
    P["T"] = T
    if T == 0:
        P["uptr"] = np.zeros(1, dtype=I64)
        return P
    # touches in sample order: (batch, feature, position in the batch, value, toff[pos] + q)
    t = np.arange(T, dtype=I64)
    tp = np.repeat(pos, m + n_aug)
    q = t - toff[tp]
    if dummies_first:
        real = q >= n_aug
        e = q - n_aug
        dummy_id = d + q
    else:
        real = q < m[tp]
        e = q
        dummy_id = d + (q - m[tp])
    src = np.where(real, indptr[samp[tp]] + e, 0)
    if len(indices):
        feat = np.where(real, indices[src], dummy_id)
        val = np.where(real, data[src], 1.0)
    else:
        feat, val = dummy_id, np.ones(T)
    b = np.searchsorted(bat_pos, tp, side="right") - 1
    pib = tp - bat_pos[b]
    key = b * I64(d + n_aug) + feat
    # a (batch, feature) group holds its touches ascending by position (stable: sample order)
    order = np.lexsort((-t if descending_positions else t, key))
    ks = key[order]
    first = np.concatenate([[True], ks[1:] != ks[:-1]])
    gstart = np.flatnonzero(first)
    gcnt = np.diff(np.concatenate([gstart, [T]]))
    gid = np.cumsum(first) - 1
    is_single_group = (gcnt <= single_max) if use_singles else np.zeros(len(gcnt), dtype=bool)
    if use_singles:
        single = np.zeros(T, dtype=np.uint8)
        single[order[is_single_group[gid]]] = 1
        P["single"] = single
    keep_g = ~is_single_group
    keep_t = keep_g[gid]
    cnt = gcnt[keep_g].astype(I64)
    gk = ks[gstart][keep_g]
    ubatch = gk // I64(d + n_aug)
    ucol = gk - ubatch * I64(d + n_aug)
    U, TM = len(cnt), int(cnt.sum())
    uptr = np.concatenate([[0], np.cumsum(cnt)]).astype(I64)
    ot = order[keep_t]
    P["U"], P["TM"] = U, TM
    P["ucol"], P["uptr"] = ucol.astype(np.int32), uptr
    P["tpos"], P["tx"] = pib[ot].astype(np.int32), val[ot]
    if want_tq:
        P["tq"] = t[ot]
    P["bat_uoff"] = np.searchsorted(ubatch, np.arange(nb + 1), side="left").astype(I64)
    P["bat_toff"] = uptr[P["bat_uoff"]]
    P["max_unique"] = int(np.diff(P["bat_uoff"]).max())
    # the count-class order: within a batch by descending min(count, clamp), feature ascending inside a class
    if sort_by_count:
        so = np.lexsort((ucol, -np.minimum(cnt, class_clamp), ubatch))
    else:
        so = np.arange(U)
    P["ucol_s"], P["ubeg_s"], P["ucnt_s"] = ucol[so].astype(np.int32), uptr[:-1][so], cnt[so].astype(np.int32)
    # heavy features
    P["bat_hoff"] = np.zeros(nb + 1, dtype=I64)
    P["bat_soff"] = np.zeros(nb + 1, dtype=I64)
    hv = np.flatnonzero(cnt > heavy_above).astype(I64)
    if len(hv):
        nseg = -(-cnt[hv] // segment)
        seg0 = np.concatenate([[0], np.cumsum(nseg)]).astype(I64)
        P["H"], P["HS"] = len(hv), int(seg0[-1])
        P["hv_u"], P["hv_seg0"] = hv, seg0
        P["bat_hoff"] = np.searchsorted(hv, P["bat_uoff"], side="left").astype(I64)
        P["bat_soff"] = seg0[P["bat_hoff"]]
        P["max_heavy"] = int(np.diff(P["bat_hoff"]).max())
        P["max_segs"] = int(np.diff(P["bat_soff"]).max())
    if use_singles or want_tq:
        P["toff"] = toff
    return P


PLAN_FIELDS = ("n_batches", "U", "T", "TM", "max_batch", "max_unique", "H", "HS", "max_heavy", "max_segs", "batch",
               "bat_pos", "bat_uoff", "bat_toff", "bat_hoff", "bat_soff",
               "perm", "ucol", "uptr", "ucol_s", "ubeg_s", "ucnt_s", "tpos", "tx", "tq", "toff", "single", "hv_u", "hv_seg0")


def plans_differ(a, b):
    """names of the fields in which two plans differ (tx as bits)"""
    bad = []
    for k in PLAN_FIELDS:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if k == "tx":
                x, y = x.view(np.uint64) if x.size else x, y.view(np.uint64) if y.size else y
            same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)
        else:
            same = int(x) == int(y)
        if not same:
            bad.append(k)
    return bad
