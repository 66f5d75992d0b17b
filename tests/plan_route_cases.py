"""Who builds a batch plan and in which instantiation (nimfm_amd/csrc/plan_route.h), restated in plain Python from what
plan.hip's comments and DESIGN.md say about the three builders: batch bounds, the width of the sort's key, twin_route,
seg_route, the rungs, and route() -- the order the driver tries them in.  Below it the case lists
tests/test_cpp_plan_route.py feeds to the header, with every threshold on both sides.  tests/plan_cases.py takes its bit
sums and natural_fl from here; tests/test_gpu_plan.py uses route() to predict what the read-back of a build reports.
No GPU, no library; plain Python integers: the numbers reach 2^63 - 1."""
import collections
import itertools

import plan_restatement

WAVE, BLOCK = 64, 256
CSC_MAX_COL, CSC_MAX_BATCHES, CSC_MAX_CELLS, CSC_MIN_FILL, CSC_FILL_LDS = 1024, 512, 2.0 ** 28, 0.5, 48 * 1024
SEG_CAP, SEG_MAX_BUCKETS, SEG_POS_BITS, SEG_FL_SHIFT, SEG_MAX_CELLS = 4096, 4096, 26, 52, 1 << 23
SEG_MIN_TOUCHES, SEG_TARGET, SEG_CHUNK = 8192.0, 2048.0, 256
CNT_CLASS_BITS = 4
KNOB_NAMES = ("NFM_PLAN_CSC", "NFM_PLAN_KEY", "NFM_PLAN_SEG", "NFM_SEG_FL", "NFM_SEG_S", "NFM_SEG_XCD")

# max_col: the dataset's longest column, known to the library once the twin is built (usable = max_col <= 1024)
Shape = collections.namedtuple("Shape", "n d max_row n_aug begin end has_order keyed_order use_singles first_singleton n_batches max_batch "
                                        "has_csc csc_built max_col seg_unfit")
Knobs = collections.namedtuple("Knobs", "csc key seg seg_fl seg_s seg_xcd", defaults=(None,) * 6)  # None: unset


def knobs_of(env):
    """the knobs as atoi reads a test's environment dict"""
    def atoi(s):
        s = s.strip()
        i = 1 if s[:1] in "+-" else 0
        j = i
        while j < len(s) and s[j].isdigit():
            j += 1
        return int(s[:j]) if j > i else 0
    return Knobs(*(atoi(env[k]) if env.get(k) is not None else None for k in KNOB_NAMES))


def ceil_log2(x, least=1):
    k = least
    while (1 << k) < x:
        k += 1
    return k


# ---------------------------------------------------------------- batch bounds
def eff_batch(ns, batch):
    """a batch longer than the range is the range"""
    return min(batch, max(ns, 1))


def batch_bounds(ns, batch, first_singleton):
    """(eff, bat_pos): the boundaries as tests/plan_restatement.py restates plan.h"""
    return eff_batch(ns, batch), [int(v) for v in plan_restatement.batch_bounds(ns, batch, first_singleton)]


def batch_counts(ns, batch, first_singleton):
    """(n_batches, max_batch) without the list"""
    eff = eff_batch(ns, batch)
    if ns == 0:
        return 0, 0
    if first_singleton:
        rest = ns - 1
        return 1 + -(-rest // eff), max(1, min(eff, rest))
    return -(-ns // eff), min(eff, ns)


# ---------------------------------------------------------------- key widths
def batch_bound(ns, batch):
    """the batch count the key's TYPE is sized for, before the boundaries exist: ceil(ns / eff) + 1"""
    eff = eff_batch(ns, batch)
    return (ns + eff - 1) // eff + 1


def key_bits(d, n_aug, n_batches):
    """(fbits, bbits, 32 | 64)"""
    f, b = ceil_log2(d + n_aug), ceil_log2(n_batches)
    return f, b, 32 if f + b <= 32 else 64


def key_bit_sum(d, n_aug, ns, batch):
    """fbits + bbits as the sort's key type is sized: features d + n_aug, batches ceil(ns / batch) + 1"""
    return ceil_log2(d + n_aug) + ceil_log2(batch_bound(ns, batch))


def count_bits(bbits):
    """the count class in the 32-bit (batch, class) key: 4 bits, fewer beyond 2^28 batches"""
    return CNT_CLASS_BITS if bbits <= 32 - CNT_CLASS_BITS else 32 - bbits


def item_bit_sum(fl, max_batch, max_row):
    return fl + ceil_log2(max_batch) + ceil_log2(max_row)


def natural_fl(d, touches_per_batch):
    """the bucket width bucketing chooses by itself: the smallest fl in 8..12 whose next width would leave fewer than
    2048 touches per cell"""
    fl = 8
    while fl < 12 and (((d - 1) >> (fl + 1)) + 1) * SEG_TARGET >= touches_per_batch:
        fl += 1
    return fl


# ---------------------------------------------------------------- the builders
def rung(v, unit):
    return 4 if v <= 4 * unit else 8 if v <= 8 * unit else 16


def off(v):
    return v is not None and v == 0


def range_ok(S):
    return S.end - S.begin >= 0 and S.begin >= 0 and (S.end <= S.n or bool(S.has_order))


def twin_route(S, K, T):
    """dense batches, no singles, no dummies, samples of the dataset, at most 512 batches and 2^28 (batch, feature) cells"""
    nbd = float(S.n_batches) * float(S.d)
    wanted = bool(not off(K.csc) and S.has_csc and not S.use_singles and S.n_aug == 0 and S.end <= S.n and S.n_batches <= CSC_MAX_BATCHES
                  and nbd <= CSC_MAX_CELLS and float(T) >= CSC_MIN_FILL * float(S.n_batches) * float(S.d))
    return dict(wanted=wanted, build_first=wanted and not S.csc_built, by_key=bool(not off(K.key) and S.keyed_order),
                tried=wanted and S.max_col <= CSC_MAX_COL)


def twin_fill(ne, n_batches):
    """k_csc_fill's workgroup: (wavefronts, ints per wavefront, bytes of LDS); four wavefronts, or two where four would
    ask for more than 48 KB (16 entries per lane; 8 entries per lane at 512 batches)"""
    per_wave = (4 * ne * WAVE + 2 * n_batches + 2) & ~1
    wpb = 2 if 4 * (BLOCK // WAVE) * per_wave > CSC_FILL_LDS else BLOCK // WAVE
    return wpb, per_wave, 4 * wpb * per_wave


def seg_route(S, K, T):
    r = dict(tried=False, fl=0, nbk=0, cells=0, S=0, cpb=0, pbits=0, qbits=0, narrow=False, sh_pos=0, sh_fl=0, qmask=0, pmask=0, xcd=0)
    bt = float(T) / float(S.n_batches)
    if not (not off(K.seg) and S.n_aug == 0 and bt >= SEG_MIN_TOUCHES and S.max_batch < 1 << SEG_POS_BITS and S.max_row < 1 << SEG_POS_BITS
            and S.d < 1 << 31 and not (S.has_csc and S.seg_unfit)):
        return r
    fl = K.seg_fl if K.seg_fl is not None and 8 <= K.seg_fl <= 12 else natural_fl(S.d, bt)
    nbk = ((S.d - 1) >> fl) + 1
    r.update(fl=fl, nbk=nbk, cells=S.n_batches * nbk)
    if not (nbk <= SEG_MAX_BUCKETS and r["cells"] <= SEG_MAX_CELLS and bt / float(nbk) <= 0.75 * SEG_CAP):
        return r
    chunk = K.seg_s if K.seg_s is not None and K.seg_s > 0 else SEG_CHUNK
    pbits, qbits = ceil_log2(S.max_batch), ceil_log2(S.max_row)
    narrow = fl + pbits + qbits <= 32
    r.update(tried=True, S=chunk, cpb=(S.max_batch + chunk - 1) // chunk, pbits=pbits, qbits=qbits, narrow=narrow, xcd=0 if off(K.seg_xcd) else 1)
    if narrow:
        r.update(sh_pos=qbits, sh_fl=qbits + pbits, qmask=(1 << qbits) - 1, pmask=(1 << pbits) - 1)
    else:
        r.update(sh_pos=SEG_POS_BITS, sh_fl=SEG_FL_SHIFT, qmask=(1 << SEG_POS_BITS) - 1, pmask=(1 << SEG_POS_BITS) - 1)
    return r


def seg_fill_lds(fl, ipt):
    NB = 1 << fl
    return 4 * (2 * NB + BLOCK * ipt) + 2 * NB


def route(S, K, T, clash=0, touches=None, h_mx=0):
    """The driver's order: the twin, else buckets, else the sort.  clash / touches: what the twin's count pass would read
    back (touches None: T); h_mx: the largest cell bucketing's count pass would read back.  Returns what the read-back of
    the build reports (builder, the instantiation fields, the dataset's state afterwards)."""
    tw, out = twin_route(S, K, T), {}
    clashed = tw["tried"] and (clash != 0 or (T if touches is None else touches) != T)
    out["csc_built"] = int(S.csc_built or tw["build_first"])
    out["seg_unfit"] = int(S.seg_unfit)
    out.update(builder="sort", csc_ne=0, csc_by_key=0, seg_fl=0, seg_nbk=0, seg_item_bits=0, seg_ipt=0, seg_s=0, seg_xcd=0, seg_max_cell=0)
    if tw["tried"] and not clashed:
        out.update(builder="twin", csc_ne=rung(S.max_col, WAVE), csc_by_key=int(tw["by_key"]))
        return out
    sg = seg_route(S, K, T)
    if sg["tried"]:
        out.update(seg_fl=sg["fl"], seg_nbk=sg["nbk"], seg_max_cell=h_mx)
        if h_mx > SEG_CAP:
            out["seg_unfit"] = int(S.seg_unfit or S.has_csc)
        else:
            out.update(builder="seg", seg_item_bits=32 if sg["narrow"] else 64, seg_ipt=rung(h_mx, BLOCK), seg_s=sg["S"], seg_xcd=sg["xcd"])
    return out


# ---------------------------------------------------------------- the cases
P26, P31 = 1 << 26, 1 << 31


def shape(d=4096, n_batches=4, max_batch=500, max_row=24, n=None, begin=0, end=None, n_aug=0, has_order=1, keyed_order=0, use_singles=0,
          first_singleton=0, has_csc=1, csc_built=1, max_col=300, seg_unfit=0):
    n = n_batches * max_batch if n is None else n
    return Shape(n, d, max_row, n_aug, begin, n if end is None else end, has_order, keyed_order, use_singles, first_singleton, n_batches,
                 max_batch, has_csc, csc_built, max_col, seg_unfit)


def route_cases():
    """(name, Shape, Knobs, T, clash, touches, h_mx): every threshold of twin_route, seg_route and the rungs on both sides"""
    out = []

    def add(name, S, K=Knobs(), T=None, clash=0, touches=None, h_mx=600):
        T = int(0.6 * S.n_batches * S.d) if T is None else T
        out.append((name, S, K, T, clash, touches, h_mx))

    # ---- the twin ----
    for nb in (1, 64, 511, 512, 513):
        add("twin_batches_%d" % nb, shape(d=8, n_batches=nb, max_batch=2))
    for nb, d in ((512, 1 << 19), (512, (1 << 19) + 1), (1, 1 << 28), (1, (1 << 28) + 1), (256, 1 << 20), (257, 1 << 20)):
        add("twin_cells_%d_x_%d" % (nb, d), shape(d=d, n_batches=nb), T=nb * d)
    for nb, d in ((4, 4096), (7, 37), (512, 8), (3, 12345)):
        half = nb * d / 2.0
        for T in (int(half) - 1, int(half), int(half) + 1, -(-nb * d // 2)):
            add("twin_fill_%d_%d_T%d" % (nb, d, T), shape(d=d, n_batches=nb), T=max(T, 1))
    for kw in (dict(n_aug=1), dict(use_singles=1), dict(has_csc=0), dict(csc_built=0), dict(csc_built=0, max_col=1025), dict(has_order=0),
               dict(keyed_order=1), dict(first_singleton=1)):
        for K in (Knobs(), Knobs(csc=0), Knobs(csc=1), Knobs(key=0), Knobs(key=1), Knobs(csc=0, key=0)):
            add("twin_%s" % "_".join("%s%d" % kv for kv in kw.items()), shape(**kw), K)
    for end in (1999, 2000, 2001, 5000):
        for has_order in (0, 1):
            add("twin_end_%d_order%d" % (end, has_order), shape(n=2000, end=end, has_order=has_order))
    add("range_begin_negative", shape(begin=-1))
    add("range_end_before_begin", shape(begin=10, end=9))
    for mc in (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5000):
        for built in (0, 1):
            for nb in (1, 100, 496, 497, 511, 512):
                add("twin_max_col_%d_built%d_nb%d" % (mc, built, nb), shape(d=8, n_batches=nb, max_batch=2, max_col=mc, csc_built=built))
    for clash, touches in ((0, None), (1, None), (0, 5), (3, 7)):
        add("twin_clash_%d_%s" % (clash, touches), shape(), clash=clash, touches=touches)
        add("twin_clash_%d_%s_small_batches" % (clash, touches), shape(max_batch=2), clash=clash, touches=touches)

    # ---- bucketing (the twin off: has_csc = 0, or n_aug, or too sparse) ----
    for nb in (1, 3, 1000):
        for T in (8191 * nb, 8192 * nb - 1, 8192 * nb, 8192 * nb + 1):
            add("seg_touches_nb%d_T%d" % (nb, T), shape(d=1 << 16, n_batches=nb), T=T)
    for mb in (P26 - 1, P26, P26 + 1):
        add("seg_max_batch_%d" % mb, shape(d=1 << 16, n_batches=2, max_batch=mb), T=40000)
    for mr in (P26 - 1, P26, P26 + 1):
        add("seg_max_row_%d" % mr, shape(d=1 << 16, n_batches=2, max_row=mr), T=40000)
    for d in (P31 - 1, P31, P31 + 1):
        add("seg_d_%d" % d, shape(d=d, n_batches=2), T=20_000_000, K=Knobs())
    for kw in (dict(n_aug=1), dict(n_aug=2), dict(seg_unfit=1), dict(seg_unfit=1, has_csc=0), dict(has_csc=0), dict(use_singles=1)):
        for K in (Knobs(), Knobs(seg=0), Knobs(seg=1), Knobs(seg=0, csc=0)):
            add("seg_%s" % "_".join("%s%d" % kv for kv in kw.items()), shape(d=1 << 16, **kw), K, T=60000)
    # the fl ladder: ((d - 1) >> (fl + 1)) + 1 buckets of the next width times 2048 against the touches per batch
    for d in (4096, 8192 - 37, 16384 - 5, 65536, 1 << 20, 1 << 24):
        for fl in range(8, 13):
            edge = (((d - 1) >> (fl + 1)) + 1) * 2048
            for bt in (edge - 1, edge, edge + 1):
                if bt >= 8192:
                    for fl_env in (None, 7, 8, 9, 10, 11, 12, 13, 0, -9):
                        add("seg_ladder_d%d_fl%d_bt%d_env%s" % (d, fl, bt, fl_env), shape(d=d, n_batches=2, has_csc=0), Knobs(seg_fl=fl_env), T=2 * bt)
    for d in ((4096 << 12) - 1, 4096 << 12, (4096 << 12) + 1, (4096 << 8), (4096 << 8) + 1):
        for fl_env in (None, 8, 12):
            add("seg_buckets_d%d_env%s" % (d, fl_env), shape(d=d, n_batches=1, has_csc=0), Knobs(seg_fl=fl_env), T=9_000_000)
    for nb, d in ((1 << 11, 1 << 24), ((1 << 11) + 1, 1 << 24), (1 << 15, 1 << 16), ((1 << 15) + 1, 1 << 16)):  # (T stays below 2^31)
        add("seg_cells_%d_x_%d" % (nb, d), shape(d=d, n_batches=nb, max_batch=16, has_csc=0), Knobs(seg_fl=8 if d <= 1 << 16 else 12), T=nb * 10000)
    for nbk_d, fl in ((4096, 12), (8192, 12), (4096, 8)):  # bt / nbk at 0.75 * kSegCap = 3072
        nbk = ((nbk_d - 1) >> fl) + 1
        for bt in (3072 * nbk - 1, 3072 * nbk, 3072 * nbk + 1):
            if bt >= 8192:
                add("seg_mean_cell_d%d_fl%d_bt%d" % (nbk_d, fl, bt), shape(d=nbk_d, n_batches=3, has_csc=0), Knobs(seg_fl=fl), T=3 * bt)
    for fl in (8, 11, 12):  # fl + pbits + qbits at 32 | 33
        for pbits in (1, 13, 14, 20):
            for over in (0, 1):
                qbits = 32 + over - fl - pbits
                if 1 <= qbits <= 26:
                    for mb, mr in itertools.product(((1 << pbits) - 1, 1 << pbits), ((1 << qbits) - 1, 1 << qbits)):
                        if mb >= 1 and mr >= 1:
                            add("seg_items_fl%d_mb%d_mr%d" % (fl, mb, mr), shape(d=1 << 16, n_batches=2, max_batch=mb, max_row=mr, n=1 << 30, has_csc=0),
                                Knobs(seg_fl=fl), T=40000)
    for h in (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 100000, (1 << 32) - 1):
        for kw in (dict(has_csc=0), dict(use_singles=1), dict(use_singles=1, seg_unfit=0)):
            add("seg_cell_%d" % h, shape(d=1 << 16, **kw), T=60000, h_mx=h)
    for s in (None, 0, -5, 1, 64, 256, 257, 1000):
        for xcd in (None, 0, 1, 2):
            for mb in (1, 63, 64, 65, 256, 257, 8193):
                add("seg_s%s_xcd%s_mb%d" % (s, xcd, mb), shape(d=1 << 16, max_batch=mb, has_csc=0), Knobs(seg_s=s, seg_xcd=xcd), T=60000)
    # a twin that clashed, then buckets; then the sort
    for h in (600, 5000):
        add("clash_then_seg_%d" % h, shape(d=64, n_batches=2, max_batch=1000, max_row=40), T=50000, clash=1, h_mx=h)
    return out


def bounds_cases():
    """(ns, batch, first_singleton)"""
    out = []
    for fs in (0, 1):
        for ns in (0, 1, 2, 3, 15, 16, 17, 33, 300, 4095, 4096):
            for batch in (1, 2, 16, 17, ns - 1, ns, ns + 1, 2 * ns + 1, 1 << 32, (1 << 32) + 7, (1 << 63) - 1):
                if batch >= 1:
                    out.append((ns, batch, fs))
    return out


def key_cases():
    """(d, n_aug, ns, batch, first_singleton): key sums at 32 | 33 by the bound, and where the bound and the count differ"""
    out = []
    for fs in (0, 1):
        for d, n_aug, ns, batch in ((1 << 20, 0, 4095, 1), (1 << 20, 0, 4096, 1), (1 << 20, 0, 4096, 4096), ((1 << 21) + 3, 0, 2000, 1),
                                    ((1 << 21) + 3, 0, 2000, 100), (1 << 20, 1, 4095, 1), ((1 << 20) - 1, 1, 4095, 1), (1 << 20, 0, 2047, 1),
                                    (1 << 20, 0, 2048, 1), (50, 0, 300, 32), (50, 2, 300, 301), (50, 0, 300, 1 << 32), (50, 0, 300, (1 << 32) + 7),
                                    (50, 0, 300, (1 << 63) - 1), (1, 0, 1, 1), (2, 0, 2, 1), (3, 0, 3, 1), ((1 << 31) - 1, 0, 2, 1), (1 << 31, 0, 2, 1),
                                    (1 << 31, 0, 3, 1), (1 << 17, 0, 1 << 15, 1), (1 << 17, 0, (1 << 15) - 1, 1), (1 << 17, 0, (1 << 15) + 1, 1)):
            out.append((d, n_aug, ns, batch, fs))
    return out
