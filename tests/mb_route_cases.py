"""What a mini-batch of the FM mini-batch driver launches, restated in Python from DESIGN.md sections 5 and 7 and the comments at
the kernels: the column kernel, the two staged streams and every grid size.  tests/test_cpp_mb_route.py holds
nimfm_amd/csrc/mb_route.h (mb_route, mb_work_bounds) against it over cases(); the row-phase half of the choice is
tests/row_slot_cases.py's, extended here by the knobs that switch modes off.

A shape, a knob set and a batch are plain namedtuples; a knob is None (unset) or the integer the variable holds."""
import collections

import numpy as np

import row_slot_cases as R

kWave, kBlock, WAVES = 64, 256, 4
SGD, ADAGRAD, PSGD = 0, 1, 2
UNSET = -2**31
STREAM_BYTES = 384 << 20
COL_KERNELS = ("phase", "strided", "sparse", "long", "long_compact", "tu1", "tu4")  # MbColKernel's order

Shape = collections.namedtuple("Shape", "L opt gen nb n_aug fit_linear d max_row avg_row n_cu use_singles first_singleton rows_ascend "
                                        "table_bytes compact_sched col_occ")
KNOBS = ("tu", "col_long", "col_long_compact", "stage_dl", "stage_w", "stage_w_passes", "col_grid",  # read per epoch call
         "stream", "singles_kernel", "held", "nq", "col_pipe", "col_wg", "col_cap_sets", "ada2")  # read once per process
Knobs = collections.namedtuple("Knobs", KNOBS, defaults=(None,) * len(KNOBS))
Batch = collections.namedtuple("Batch", "b len uniq touches heavy segs")


def line(request, S, K, B):
    """one input line of tests/cpp/mb_route_test.cpp"""
    return " ".join([str(request)] + [repr(float(v)) if f == "avg_row" else str(int(v)) for f, v in zip(S._fields, S)] +
                    [str(UNSET if v is None else v) for v in K] + [str(v) for v in B])


def cdiv(a, b):
    return -(-a // b)


def chosen_split(L, n, avg_row, n_cu, request=0):
    """row slots per sample (choose_split, lane_map.h): the request where NFM_SPLIT is set; else enough wavefronts to fill the chip
    (16 per CU) and at most ~8 rounds of loads per lane, within the 64 / L slots of a wavefront and 16"""
    if request >= 1:
        return R.requested_split(L, request)
    s = max(R.p2(n_cu * 16.0 * kWave / (max(n, 1) * L)), R.p2(avg_row / 32.0))
    return max(1, min(s, kWave // L, 16))


def route(S, K, B, request=0):
    """dict of what the batch launches; 'bad_passes': True where NFM_STAGE_W_PASSES must be refused (nothing else is compared then)"""
    L, per_wave = S.L, kWave // S.L
    sgd, ada, psgd = S.opt == SGD, S.opt == ADAGRAD, S.opt == PSGD
    o = {}
    o["use_stored"] = psgd or (ada and bool(S.first_singleton) and B.b == 0)
    have_singles = not S.gen and bool(S.use_singles)
    own_kernel = K.singles_kernel is not None and K.singles_kernel != 0
    o["singles_in_row"], o["singles_in_col"] = have_singles and not own_kernel, have_singles and own_kernel
    # rows streamed: tables beyond 384 MB in a batch with singles; NFM_STREAM=0|1 overrides
    o["stream_rows"] = (K.stream != 0) if K.stream is not None and K.stream >= 0 else (have_singles and S.table_bytes > STREAM_BYTES)
    # ---- row phase
    widest = S.max_row + S.n_aug
    slots = R.ladder(chosen_split(L, B.len, S.avg_row, S.n_cu, request), per_wave)
    cap = R.held_capacity(L, slots)
    if K.held == 0 or cap == 0 or S.nb == 0:
        mode = 0  # streamed
    elif widest > cap:
        mode = 3  # chunks of held entries
    elif not S.gen and K.nq != 0 and sgd and o["singles_in_row"] and L * slots == kWave:
        mode = 2  # register-resident rows
    else:
        mode = 1
    if ada and not S.gen and L == 32 and K.ada2 != 0 and o["singles_in_row"] and not o["use_stored"] and widest <= 64:
        o.update(row="ada2", slots=2, mode=0, sing=False, nA=cdiv(B.len, 2))  # two wavefronts per sample
    else:
        samples_per_block = WAVES * (kWave // (L * slots))
        o.update(row="row", slots=slots, mode=4 if mode == 2 and o["stream_rows"] else mode, sing=mode == 0 and o["singles_in_row"],
                 nA=cdiv(B.len, samples_per_block))
    o["nS"] = cdiv(B.len, WAVES) if o["singles_in_col"] else 0  # k_singles: one wavefront per sample
    # ---- column phase: L lanes per feature; beyond cap_sets resident sets ONE resident set of workgroups that stride
    tu = 2 if K.tu is None else K.tu
    blocks = cdiv(B.uniq, WAVES * per_wave)
    wg_per_cu = S.col_occ if K.col_wg is None else K.col_wg
    sets = 4 if K.col_cap_sets is None else K.col_cap_sets
    grid = 0 if K.col_grid is None else K.col_grid
    capped = tu == 2 and ((wg_per_cu > 0 and blocks > sets * S.n_cu * wg_per_cu) or (grid > 0 and blocks > grid))
    if capped:
        blocks = min(blocks, grid) if grid > 0 else S.n_cu * wg_per_cu
    o["nB"] = blocks + 1  # + the closing workgroup
    pipelined = K.col_pipe != 0 and not S.gen and S.nb == 1 and not psgd
    if not pipelined or tu != 2 or K.col_long == 0:
        long = False
    elif K.col_long is not None:
        long = True
    else:  # by itself: 33-64 factors, a strided batch, four touches per feature or more on average
        long = capped and L == 32 and B.touches >= 4.0 * B.uniq
    compact = K.col_long_compact != 0 and bool(S.compact_sched)
    if tu in (1, 4) and not psgd:
        o["col"] = "tu%d" % tu
    elif long:
        o["col"] = "long_compact" if compact else "long"
    elif capped:
        o["col"] = "sparse" if pipelined else "strided"
    else:
        o["col"] = "phase"
    # ---- the two staged streams
    o["stage_dl"] = long and compact and K.stage_dl != 0 and B.touches > 0
    o["dl_grid"] = min(cdiv(B.touches, 4 * kBlock), S.n_cu * 32) if o["stage_dl"] else 0
    can_w = sgd and not S.gen and bool(S.fit_linear) and mode == 1 and compact
    stage_w = can_w and K.stage_w != 0 and (K.stage_w is not None or long)
    o.update(stage_w="gather", w_cap=cap, w_parts=0, w_wg=0, w_slice=0, bad_passes=False)
    if stage_w:
        passes = (4 if S.rows_ascend else 0) if K.stage_w_passes is None else K.stage_w_passes
        if passes != 0:
            o["stage_w"] = "ranges"
            if passes < 0 or passes > cap or passes & (passes - 1):
                o["bad_passes"] = True
                return o
            parts, per_step = passes, kWave // (cap // passes)  # cap / passes lanes per sample
        else:
            o["stage_w"] = "slices"
            parts = max(1, cdiv(8 * S.d, 2 << 20))  # a slice's weights: 2 MB of an L2
            o["w_slice"] = cdiv(S.d, parts)
            per_step = kWave // cap
        o["w_parts"] = parts
        o["w_wg"] = max(1, min(cdiv(cdiv(B.len, per_step), WAVES), S.n_cu * 8))
    # ---- heavy features: L lanes per segment, then one wavefront per feature
    heavy = S.nb > 0 and B.heavy > 0
    o["nsb"] = cdiv(B.segs, WAVES * per_wave) if heavy else 0
    o["nH"] = cdiv(B.heavy, WAVES) if heavy else 0
    return o


def parse(out_line):
    """one output line of tests/cpp/mb_route_test.cpp as the dict route() gives, plus 'held', 'cap', 'bounds', 'counters'"""
    f = out_line.split()
    v = [int(x) for x in f[:22]]
    names = ("use_stored", "row", "slots", "mode", "sing", "stream_rows", "nA", "singles_in_row", "singles_in_col", "nS", "stage_w", "w_cap",
             "w_parts", "w_wg", "w_slice", "bad_passes", "stage_dl", "dl_grid", "col", "nB", "nsb", "nH")
    o = dict(zip(names, v))
    for k in ("use_stored", "sing", "stream_rows", "singles_in_row", "singles_in_col", "bad_passes", "stage_dl"):
        o[k] = bool(o[k])
    o["row"] = ("row", "ada2")[o["row"]]
    o["stage_w"] = ("gather", "slices", "ranges")[o["stage_w"]]
    o["col"] = COL_KERNELS[o["col"]]
    assert f[22] == "|" and f[25] == "|" and f[30] == "|"
    o["held"], o["cap"] = int(f[23]), int(f[24])
    o["bounds"] = dict(zip(("partsA", "partsB", "dLt", "Wt"), (int(x) for x in f[26:30])))
    o["counters"] = (f[31], f[32])
    return o


# ---------------------------------------------------------------- the grid
LENS = (1, 2, 3, 4, 5, 255, 256, 257, 8192, 262144)
WIDEST = (0, 1, 31, 32, 33, 63, 64, 65, 129)
TRI = (None, 0, 1)
KNOB_VALUES = dict(tu=(None, 1, 2, 4), col_long=TRI, col_long_compact=TRI, stage_dl=TRI, stage_w=TRI, stage_w_passes=(None, 0, 1, 4, 64, 3),
                   col_grid=(None, 0, 2, 3), stream=TRI, singles_kernel=TRI, held=TRI, nq=TRI, col_pipe=TRI, col_wg=TRI, col_cap_sets=TRI,
                   ada2=TRI)


def cases(n_default=20000, n_knobs=60000, n_staged=4000, seed=11):
    """[(Shape, Knobs, Batch)]: draws from the cross product of the values at which a choice changes -- every lane width, the three
    optimizers, row lengths either side of 32 and 64 held entries, batch lengths either side of a workgroup's samples, feature
    counts either side of the grid cap, touches either side of four per feature, tables either side of 384 MB -- the first
    n_default with every knob unset, the next n_knobs with every knob drawn from its values (unset half of the time), the last
    n_staged the same but SGD with one order of degree 2, a fitted linear term and NFM_STAGE_W=1: the corner in which the linear
    weights are staged, where NFM_STAGE_W_PASSES, the slices and the strides of 32 and 64 are decided.  The cross product itself has more than 1e15 members; test_cpp_mb_route.py asserts that the draw reaches every value of every axis and
    every outcome."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_default + n_knobs + n_staged):
        pick = lambda vals: vals[int(rng.integers(len(vals)))]
        L = pick((1, 2, 4, 8, 16, 32, 64))
        opt, nb, n_aug = pick((SGD, ADAGRAD, PSGD)), pick((0, 1, 1, 2)), pick((0, 1))
        gen = 1 if nb != 1 else pick((0, 0, 1))  # one order: degree 2 or higher
        widest = max(pick(WIDEST), n_aug)
        n_cu, col_occ = pick((1, 8, 256)), pick((1, 5, 8))
        if i < n_default:
            K = Knobs()
        else:
            K = Knobs(**{k: (None if rng.integers(2) else pick(v)) for k, v in KNOB_VALUES.items()})
        S = Shape(L, opt, gen, nb, n_aug, pick((0, 1)), pick((1, 1000, 262144, 262145, 3000000)), widest - n_aug, pick((0.0, 10.5, 39.0, 100.0)),
                  n_cu, pick((0, 1)), pick((0, 1)), pick((0, 1)), STREAM_BYTES + pick((0, 8)), pick((0, 1)), col_occ)
        if i >= n_default + n_knobs:
            S, K = S._replace(opt=SGD, gen=0, nb=1, fit_linear=1, compact_sched=1), K._replace(stage_w=1, held=None, col_long_compact=None)
        # features either side of the cap of the grid this shape gets (with the knobs' own workgroups per CU and sets where given)
        wg = col_occ if K.col_wg is None else K.col_wg
        sets = 4 if K.col_cap_sets is None else K.col_cap_sets
        at_cap = max(sets * n_cu * wg, 1) * WAVES * (kWave // L)
        uniq = pick((0, 1, 7, WAVES * (kWave // L) * 3, at_cap, at_cap + 1, 2 * at_cap + 5))
        touches = max(0, pick((4 * uniq, 4 * uniq - 1, uniq, 0)))
        heavy = pick((0, 0, 1, 5))
        out.append((S, K, Batch(pick((0, 0, 1, 7)), pick(LENS), uniq, touches, heavy, 3 * heavy)))
    return out
