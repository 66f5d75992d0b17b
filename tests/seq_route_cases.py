"""Which kernels one call of NFM_MODE_SEQUENTIAL takes, restated in plain Python from the lines of seqwin.hip
(seq_window_view, seq_window_supported, launch_sequential_window), api.hip (seq_window_offered) and seq.hip (launch_sequential)
as they stood before nimfm_amd/csrc/seq_route.h gathered them: win_route() and one_wg_route() below, and the case lists
tests/test_cpp_seq_route.py feeds to the header.  The workers' LDS bytes are the host's formulas of before seqwin_layout.h
(tests/cpp/seqwin_layout_test.cpp holds that header to the same ones).  No GPU, no library: tests/test_gpu_seq_route.py uses
the same two functions to predict which counter a call bumps."""
import collections
import itertools

FM, FFM = 0, 1  # NFM_KIND_FM, NFM_KIND_FFM
WAVE, LDS_MAX, LDS_FLOOR = 64, 160 * 1024, 81 * 1024
WIN_RING, WIN_DEPTH, WIN_HDR, WIN_MAX_NL, SUM_GRAN, SUM_RING, RES_WORDS = 8, 8, 4, 5, 13, 256, 4
FW_SLOT = 64 * 4 + 3 * 64 * 64 * 2 + 5 * 64 * 2  # granules of a worker's forwarding area per buffer set
SUPPORT_W, SUPPORT_W_SLOTS = 256, 128  # the worker counts the support check assumes
WIN_MAX_DEG, SEQ_MAX_DEG = 6, 8
PIPE_THREADS, PIPE_WIDE, PIPE_PAIR_CAP = 256, 512, 4096
WORKERS = ("general", "k64", "ffm", "fmx")  # WK_*
REASONS = ("ok", "off", "kp", "shape", "mail", "lds", "limits", "cus", "short")  # WinReason
STEPS = ("pipe", "staged", "plain")  # SeqStep
REFUSALS = ("ok", "kp", "degree")  # SeqRefusal

Shape = collections.namedtuple("Shape", "kind degree nb kc k Kp n_aug fit_intercept d da bs rs m_cap ns nnz ada n_cu")
Knobs = collections.namedtuple("Knobs", "win exact nocond w par trace pipe stage", defaults=(None,) * 8)  # None: unset


def lanes_for_k(k):
    """lanes per row of a k-factor block: the power of two >= ceil(k / 2), at most 64 (common.h); Kp = 2 L"""
    L = 1
    while L < (k + 1) // 2 and L < 64:
        L *= 2
    return L


def fm_shape(k, degree=2, orders=1, m_cap=8, fit_intercept=1, ada=0, ns=4096, n_cu=256, d=1000, n_aug=0, nnz=None):
    """a FactorizationMachine as api.hip lays it out: k <= 128: `orders` order-major blocks; beyond: one order in kc blocks of
    128, feature-major (wide_rows)"""
    da = d + n_aug
    nnz = ns * max(m_cap - n_aug, 0) if nnz is None else nnz
    if k > 128:
        assert orders == 1
        kc = -(-k // 128)
        return Shape(FM, degree, kc, kc, 128, 128, n_aug, fit_intercept, d, da, 1, kc, m_cap, ns, nnz, ada, n_cu)
    return Shape(FM, degree, orders, 1, k, 2 * lanes_for_k(k), n_aug, fit_intercept, d, da, da, 1, m_cap, ns, nnz, ada, n_cu)


def ffm_shape(k, F, m_cap=8, fit_intercept=1, ada=0, ns=4096, n_cu=256, d=1000, nnz=None):
    nnz = ns * m_cap if nnz is None else nnz
    return Shape(FFM, 2, F, 1, k, 2 * lanes_for_k(k), 0, fit_intercept, d, d, 1, F, m_cap, ns, nnz, ada, n_cu)


def row_view(S):
    """seq_row_view (opt_views.h): what the one-workgroup kernels are given -- a wide FM as ONE row of kc * 128 factors"""
    if not (S.kind == FM and S.kc > 1 and S.nb == S.kc and S.bs == 1 and S.rs == S.nb):
        return S
    return S._replace(Kp=S.nb * S.Kp, k=S.nb * S.Kp, nb=1, kc=1, bs=S.da, rs=1)


def lg(Kp):
    n = 1
    while (1 << n) < Kp:
        n += 1
    return n


def padded(Kp, rows):
    grp = (WAVE >> lg(Kp)) * 4
    return -(-rows // grp) * grp


def worker_lds(worker, Kp, nb, m_cap, ada, W):
    """bytes of LDS a worker asks for: the four formulas the host had before seqwin_layout.h"""
    a = 4 if ada else 2
    if worker == "k64":
        return 8 * ((3 if ada else 1) * WAVE * WAVE + WAVE) + 4 * W
    if worker == "general":
        mcp = padded(Kp, m_cap)
        return 8 * (a * mcp * Kp + WAVE + a * mcp) + 4 * 3 * mcp + 4 * W
    mcs = padded(Kp, m_cap * nb)
    if worker == "ffm":
        return 8 * (a * mcs * Kp + m_cap * m_cap + 4 * WAVE + 4 + a * m_cap) + 8 * 2 + 4 * (5 * m_cap + nb + nb * m_cap) + 4 * W + 64
    return 8 * (a * mcs * Kp + WAVE + 4 * WAVE + 3 * WIN_MAX_DEG * WAVE + 4 + a * m_cap) + 8 * 3 + 4 * 4 * m_cap + 4 * W + 64


def two_block(S, K):
    """seq_window_view's predicate: a degree-2 FM whose rows are 128 doubles, read as blocks of 64"""
    if K.exact not in (None, 0):
        return False
    if not (S.kind == FM and S.degree == 2 and S.n_aug == 0 and S.Kp == 128):
        return False
    one_block = S.nb == 1 and S.kc == 1 and S.bs == S.da and S.rs == 1
    wide_rows = S.kc > 1 and S.nb == S.kc and S.bs == 1 and S.rs == S.nb
    return one_block or wide_rows


def win_route(S, K, fallbacks=0, snap_bytes=0):
    r = {"two_block": int(two_block(S, K))}
    nb, Kp = (2 * S.nb, 64) if r["two_block"] else (S.nb, S.Kp)
    r.update(nb=nb, Kp=Kp)
    exact = K.exact not in (None, 0)
    no_cond = K.nocond != 0 and not S.fit_intercept
    one_term = not no_cond and not exact
    ffm = S.kind == FFM
    fmx = S.kind == FM and (nb != 1 or S.degree != 2)
    mode = 1 if K.win is None else K.win
    term_mail = not (no_cond or one_term)

    def mail_full(terms):
        return term_mail and WIN_HDR + -(-terms // 64) * 64 > WAVE * WIN_MAX_NL

    def reason():
        m = S.m_cap
        if mode == 0:
            return "off"
        if Kp > 64 or Kp < 2:
            return "kp"
        if ffm:
            if S.n_aug != 0 or nb < 1 or m < 1:
                return "shape"
            if mail_full(m + m * (m - 1) // 2):
                return "mail"
            if worker_lds("ffm", Kp, nb, m, S.ada, SUPPORT_W_SLOTS) > LDS_MAX:
                return "lds"
        elif fmx:
            if S.n_aug != 0 or nb < 1 or S.degree < 2 or S.degree > WIN_MAX_DEG or m < 1:
                return "shape"
            if mail_full(m + nb):
                return "mail"
            if worker_lds("fmx", Kp, nb, m, S.ada, SUPPORT_W_SLOTS) > LDS_MAX:
                return "lds"
        else:
            if S.kind != FM or nb != 1 or S.degree != 2 or S.n_aug != 0:
                return "shape"
            if mail_full(m):
                return "mail"
            if not (Kp == 64 and m <= 64) and worker_lds("general", Kp, nb, m, S.ada, SUPPORT_W) > LDS_MAX:
                return "lds"
        if S.nnz >= 2 ** 32 or S.d >= 2 ** 31 or S.ns >= 2 ** 31:
            return "limits"
        if S.n_cu < 17:
            return "cus"
        return "ok" if mode == 2 or S.ns >= 2048 else "short"

    r["reason"] = reason()
    r["supported"] = int(r["reason"] == "ok")
    snap_pays = K.win == 2 or S.ns * 0.8e-6 * 0.25 >= snap_bytes / 2.0e12
    r["offered"] = int(snap_pays and fallbacks < 2 and r["supported"])
    r.update(no_cond=int(no_cond), one_term=int(one_term))
    if not r["supported"]:
        return r
    m_cap = max(S.m_cap, 1)
    k64 = not ffm and not fmx and Kp == 64 and m_cap <= 64
    worker = "ffm" if ffm else "fmx" if fmx else "k64" if k64 else "general"
    W = 128 if no_cond or k64 else 64
    if no_cond and k64 and fallbacks == 0:
        W = 256
    if K.w is not None:
        W = K.w
    lgW = 4
    while (2 << lgW) <= W and lgW < (8 if no_cond else 7):
        lgW += 1
    W = 1 << lgW
    first_worker = 0 if no_cond else 1
    while W + first_worker > S.n_cu and lgW > 4:
        lgW -= 1
        W = 1 << lgW
    fits_cus = W > WIN_DEPTH and W + first_worker <= S.n_cu
    terms = m_cap + m_cap * (m_cap - 1) // 2 if ffm else m_cap + nb if fmx else m_cap
    ch = 32 if one_term or terms <= 32 else 64
    FW = WIN_HDR + 32 if one_term else WIN_HDR + -(-terms // ch) * ch
    np_ = 4 if no_cond else 2
    lds_worker = worker_lds(worker, Kp, nb, m_cap, S.ada, W)
    lds_cond = 8 * (2 + 9 * SUM_RING) + 4 * SUM_RING if one_term else 8 * 2 + 8 * WIN_RING * FW
    lds = max(lds_worker, lds_cond)
    r.update(worker=worker, counter="seq_route_win_" + worker, W=W, lgW=lgW, first_worker=first_worker, m_cap=m_cap, lgKp=lg(Kp),
             terms=terms, ch=ch, FW=FW, np=np_, thr=np_ - 1, near_r=W, par_min=6 if K.par is None else K.par,
             lds_worker=lds_worker, lds_cond=lds_cond, lds_bytes=max(lds, LDS_FLOOR),
             n_fwd=SUM_GRAN * np_ * W if one_term else W * np_ * FW, n_res=W * np_ * RES_WORDS, n_ctl=W + 64, n_partial=2 * (W + 1),
             n_fw=(FW_SLOT * np_ + 2 * WAVE) * W, n_fw_tags=FW_SLOT * np_ * W, n_scales=0 if S.ada else 2 * S.ns,
             fits_cus=int(fits_cus), fits=int(fits_cus and lds <= LDS_MAX))
    return r


def one_wg_route(S, K):
    """launch_sequential's choice for the model as seq_row_view gives it"""
    if S.Kp > 1024:
        return {"refusal": "kp"}
    ffm = S.kind == FFM
    if not ffm and S.degree > SEQ_MAX_DEG:
        return {"refusal": "degree"}
    T = max(-(-S.Kp // WAVE) * WAVE, WAVE)
    m_cap = max(S.m_cap, 1)
    r = {"refusal": "ok", "T": T, "m_cap": m_cap}
    if K.pipe != 0 and (ffm or (S.nb == 1 and S.degree == 2)) and 1 <= S.nb < 32768 and m_cap <= PIPE_THREADS:
        lgS = max(lg(S.Kp), 1)
        Sp = 1 << lgS
        nbk = S.nb if ffm else 1
        slots = nbk * m_cap
        threads = PIPE_THREADS
        G = threads // Sp if Sp <= threads else 0
        rc = -(-slots // G) if G > 0 else 1 << 30
        if G > 0 and rc >= 8 and -(-slots // (2 * G)) <= 16:
            threads, G = PIPE_WIDE, 2 * G
            rc = -(-slots // G)
        pair = m_cap * m_cap if ffm and m_cap * m_cap <= PIPE_PAIR_CAP else 0
        base = threads + 2 * slots * Sp + 7 * m_cap + pair
        tail = 8 * 3 * m_cap + 4 * (m_cap + (3 * m_cap + nbk + nbk * m_cap if ffm else 0))
        split = int(not ffm and 8 * (base + m_cap * Sp) + tail <= LDS_MAX)
        nbytes = 8 * (base + (m_cap * Sp if split else 0)) + tail
        if G >= 1 and rc <= 64 and nbytes <= LDS_MAX:
            rungs = (2, 4, 8, 16) if threads == PIPE_WIDE else (1, 2, 4, 8, 16, 32, 64)
            r.update(step="pipe", threads=threads, S=Sp, lgS=lgS, rc=min(g for g in rungs if g >= rc), split_terms=split, lds_bytes=nbytes,
                     table_in_lds=1, table_bytes=0, counter="seq_route_pipe_wide" if threads == PIPE_WIDE else "seq_route_pipe")
            return r
    table = 8 * max(S.nb, 1) * m_cap * T
    in_lds = 8 * T + table <= LDS_MAX
    nbytes = 8 * T + (table if in_lds else 0)
    staged = nbytes + table + 8 * 3 * m_cap
    r.update(threads=T, S=0, lgS=0, rc=0, split_terms=0, table_in_lds=int(in_lds), table_bytes=table)
    if not ffm and in_lds and K.stage != 0 and S.nb > 0 and staged <= LDS_MAX:
        r.update(step="staged", lds_bytes=staged, counter="seq_route_staged")
    else:
        r.update(step="plain", lds_bytes=nbytes, counter="seq_route_plain" if in_lds else "seq_route_plain_scratch")
    return r


# ---------------------------------------------------------------------------------------------------------------- the case lists
KPS = (2, 4, 8, 16, 32, 64, 128)
M_CAPS = (0, 1, 31, 32, 33, 63, 64, 65, 252, 253, 316, 317, 1000)
WS = (None, 1, 8, 16, 100, 128, 256, 1000)
N_CUS = (16, 17, 64, 65, 128, 129, 256, 257, 304)
TRI = (None, 0, 1)


def families(Kp, m_cap, fi, ada, **kw):
    """every model family at rows of Kp doubles: (name, Shape).  k = Kp / 2 + 1 ... Kp factors pad to Kp; the two-block view and
    the wide rows exist at Kp = 128 only"""
    k = Kp if Kp > 2 else 1
    a = dict(m_cap=m_cap, fit_intercept=fi, ada=ada, **kw)
    out = [("deg2", fm_shape(k, **a))]
    if Kp == 128:
        out += [("two_block_%d" % kk, fm_shape(kk, **a)) for kk in (65, 100, 128)]
        out += [("wide_%d" % kk, fm_shape(kk, **a)) for kk in (129, 200, 300, 1000)]
        out += [("deg2_aug", fm_shape(k, n_aug=1, **a))]  # augmented features: no view, no window
    # several orders / degree >= 3; degree 7 is beyond the workers'; two blocks of degree 2: what the view makes
    out += [("orders_%d_deg%d" % (o, g), fm_shape(min(k, 128), degree=g, orders=o, **a)) for g in (2, 3, 4, 5, 6, 7)
            for o in sorted({1, 2, g - 1}) if 1 <= o <= max(g - 1, 2) and (g, o) != (2, 1)]
    out += [("ffm_F%d" % F, ffm_shape(k, F, **a)) for F in (1, 2, 16, 39, 64)]
    return out


def support_grid():
    """which flavour, which worker, supported or why not: families x Kp x m_cap x intercept x optimizer x _EXACT x _NOCOND, at
    NFM_SEQ_WIN=2 on 256 CUs"""
    for Kp, m_cap, fi, ada, exact, nocond in itertools.product(KPS, M_CAPS, (0, 1), (0, 1), TRI, TRI):
        for name, S in families(Kp, m_cap, fi, ada):
            yield name, S, Knobs(win=2, exact=exact, nocond=nocond), 0, 0


def worker_models():
    """one model per worker, and two whose four-wavefront worker asks for 160 KiB less a few hundred bytes at the 128 workers the
    support check assumes (AdaGrad's field-aware one, SGD's several-orders one): 256 workers' counters are 512 bytes more"""
    return [("k64", fm_shape(64, m_cap=64)), ("general_kp16", fm_shape(16, m_cap=32)), ("general_long", fm_shape(64, m_cap=65)),
            ("fmx", fm_shape(8, degree=3, orders=2, m_cap=24)), ("two_block", fm_shape(100, m_cap=40)), ("ffm", ffm_shape(8, 16, m_cap=16)),
            ("ffm_lds_edge", ffm_shape(8, 39, m_cap=15)), ("fmx_lds_edge", fm_shape(16, degree=6, orders=5, m_cap=113))]


def worker_grid():
    """the worker count: models x NFM_SEQ_WIN_W x CUs x earlier aborts x intercept x _NOCOND x optimizer"""
    for (name, S), w, n_cu, fb, fi, nocond, ada in itertools.product(worker_models(), WS, N_CUS, (0, 1, 2), (0, 1), TRI, (0, 1)):
        yield name, S._replace(n_cu=n_cu, fit_intercept=fi, ada=ada), Knobs(win=2, w=w, nocond=nocond), fb, 0


def pays(ns):
    """the largest snapshot that still pays for ns samples (bytes), by the rule's own constants"""
    b = int(ns * 0.8e-6 * 0.25 * 2.0e12)
    while ns * 0.8e-6 * 0.25 >= (b + 1) / 2.0e12:
        b += 1
    while not ns * 0.8e-6 * 0.25 >= b / 2.0e12:
        b -= 1
    return b


def offer_grid():
    """offered or not: NFM_SEQ_WIN x samples x earlier aborts x the snapshot on either side of the pays rule x CUs, and the
    2^31 / 2^32 limits"""
    for (name, S), win, ns, fb, side, n_cu in itertools.product(worker_models()[:4], (None, 0, 1, 2), (2047, 2048, 100000), (0, 1, 2), (0, 1),
                                                                (16, 17, 256)):
        yield name, S._replace(ns=ns, n_cu=n_cu, nnz=ns * 8), Knobs(win=win), fb, pays(ns) + side
    for (name, S), (nnz, d, ns) in itertools.product(worker_models()[:4], [(2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 32, 1000, 4096),
                                                                           (4096, 2 ** 31, 4096), (4096, 1000, 2 ** 31)]):
        yield name, S._replace(nnz=nnz, d=d, da=d, bs=d if S.bs != 1 else 1, ns=ns), Knobs(win=2), 0, 0
    for (name, S), par, trace in itertools.product(worker_models()[:2], (None, 0, 6, 9), TRI):
        yield name, S, Knobs(win=2, par=par, trace=trace), 0, 0


def window_cases():
    return list(support_grid()) + list(worker_grid()) + list(offer_grid())


def one_wg_cases():
    """(name, Shape as seq_row_view gives it, Knobs): Kp 2 ... 1024 and 1025, rows across 256 / 257, every rc rung, the switch to
    512 threads, the pair table's cap, the 160 KiB edges of split_terms, the staged step and the table's placement"""
    out = []
    kps = (2, 4, 8, 16, 32, 64, 128, 192, 256, 320, 512, 1000, 1024, 1025)
    ms = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 330, 1000)
    for Kp, m, ada, pipe, stage in itertools.product(kps, ms, (0, 1), (None, 0, 1), (None, 0, 1)):
        base = Shape(FM, 2, 1, 1, Kp, Kp, 0, 1, 1000, 1000, 1000, 1, m, 4096, 4096 * m, ada, 256)
        K = Knobs(pipe=pipe, stage=stage)
        out.append(("deg2", base, K))
        out += [("orders_%d_deg%d" % (o, g), base._replace(degree=g, nb=o), K) for g, o in ((2, 0), (3, 1), (3, 2), (6, 5), (8, 3), (9, 1))]
        if Kp <= 128:
            out += [("ffm_F%d" % F, base._replace(kind=FFM, nb=F, bs=1, rs=F), K) for F in (1, 2, 3, 16, 39, 64, 200)]
    # the 160 KiB edges, one row either side: found by walking m at the widths where they exist
    for Kp, nb in ((64, 1), (128, 1), (256, 1), (64, 2), (1024, 1), (512, 3)):
        for m in range(1, 400):
            out.append(("edge", Shape(FM, 2 if nb == 1 else 3, nb, 1, Kp, Kp, 0, 1, 1000, 1000, 1000, 1, m, 4096, 4096 * m, 0, 256), Knobs(pipe=0)))
            out.append(("edge", Shape(FM, 2 if nb == 1 else 3, nb, 1, Kp, Kp, 0, 1, 1000, 1000, 1000, 1, m, 4096, 4096 * m, 0, 256), Knobs()))
    for F, m in itertools.product((2, 16, 39), range(1, 130)):  # the pair table's cap at m = 64 / 65, field-aware rungs
        out.append(("ffm_walk", Shape(FFM, 2, F, 1, 8, 8, 0, 1, 1000, 1000, 1, F, m, 4096, 4096 * m, 0, 256), Knobs()))
    return out
