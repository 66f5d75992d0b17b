// nimfm_amd/csrc/seq_route.h -- which kernel a call of NFM_MODE_SEQUENTIAL takes, with how many workgroups, threads and bytes of
// LDS, decided once per epoch call as pure functions: win_route(shape, knobs, fallbacks, snap_bytes) for the dependency window
// (seqwin.hip) and seq_one_wg_route(shape, knobs) for the one-workgroup kernels (seq.hip).  seq_epoch (api.hip) builds shape and
// knobs, offers the window by the first and hands it to launch_sequential_window, which sizes its buffers and fills WinArgs from
// it; launch_sequential dispatches on the second.  Plain C++17, no HIP header: tests/cpp/seq_route_test.cpp holds both against
// the restatement of tests/seq_route_cases.py and against a copy of the lines they replaced, with g++ alone.  Why each choice is
// what it is: the comments at the kernels (seqwin.hip, seq.hip) and DESIGN.md's sections on the window.
//
// The environment knobs of the driver, all read by seq_knobs() and nowhere else:
//   knob                    read          what it overrides (unset = the default)
//   NFM_SEQ_WIN             per call      0: never the window; 2: whenever the shape is supported (no "does it pay" rules: fewer
//                                         than 2048 samples, a snapshot that costs more than a quarter of the call); unset or
//                                         anything else: when it pays
//   NFM_SEQ_WIN_EXACT       per call      anything but 0: the term-by-term chain where the intercept is fitted (the reference's
//                                         rounding), and no two-blocks-of-64 view of a 65 ... 128-factor model; unset: one-term
//   NFM_SEQ_WIN_NOCOND      per call      0: a conductor even where the intercept is not fitted; unset: none there
//   NFM_SEQ_WIN_W           per call      workers asked for: rounded down to a power of two in [16, 128] (256 without a conductor),
//                                         then halved until they fit the CUs; unset: 64, 128 or 256 by shape (win_route)
//   NFM_SEQ_WIN_PAR         per call      the shortest chunk the one-term conductor solves in parallel, 0: never; unset: 6
//   NFM_SEQ_WIN_TRACE       per call      anything but 0: wall-clock stamps of the first launch's samples (debugging)
//   NFM_SEQ_WIN_TRACE_FILE  per call      where the stamps go; unset: /tmp/seqwin_trace.bin
//   NFM_SEQ_PIPE            per process   0: never the pipelined step (k_sequential_pipe)
//   NFM_SEQ_STAGE           per process   0: never the staged step (k_sequential<.., STAGE = true>)
// "per call": at every epoch call (tests flip them inside one process); "per process": at the first one.
// The hooks build (-DNFM_TEST_HOOKS) reads two fault-injection variables of its own where they act (seqwin.hip, api.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mb_route.h"  // kKnobUnset, mb_knob
#include "seqwin_layout.h"

namespace nfm {

enum { SEQ_KIND_FM = 0, SEQ_KIND_FFM = 1 };  // = NFM_KIND_FM, NFM_KIND_FFM (nimfm_hip.h; asserted in opt_views.h)
constexpr size_t kSeqLdsMax = 160 * 1024;    // of a CU

// ---- the window's constants (seqwin.hip says what each is for) ----
constexpr int kWinRing = 8;    // LDS ring slots between the conductor's fetch and chain wavefronts (power of two)
constexpr int kWinDepth = 8;   // mailboxes the fetch wavefront has requested ahead (must stay < W)
constexpr int kWinHdr = 4;     // mailbox tail, after the MC term slots: anova sum, target, eta(alpha0) | eta0 (it-1) alpha0, number of chain terms
constexpr int kWinMaxNL = 5;   // 64-lane loads per mailbox: rows of up to 316 entries
constexpr int kSumGran = 13;   // granules of a one-term mailbox (seqwin.hip: post_sum)
constexpr int kSumRing = 256;  // the one-term conductor's LDS ring, in samples (a power of two >= 2 W)
constexpr int kResWords = 4;   // conductor -> worker: {dL, yhat} as tagged granules (several workers may read them)
// a worker's forwarding area (seqwin.hip: "A worker's forwarding area"), in granules
constexpr int kFwVals = 3;
constexpr size_t kFwRows = (size_t)kWinLdsWave * 4;                                      // granules of a1 and T
constexpr size_t kFwLin = kFwRows + (size_t)kFwVals * kWinLdsWave * kWinLdsWave * 2;     // start of the per-entry part
constexpr size_t kFwSlot = kFwLin + (size_t)5 * kWinLdsWave * 2;                         // granules per (worker, parity)
constexpr size_t kWinLdsFloor = 81 * 1024;  // more than half of a CU's LDS: one workgroup per CU
enum { WK_GENERAL = 0, WK_K64 = 1, WK_FFM = 2, WK_FMX = 3 };  // which worker

// ---- the one-workgroup kernels' constants (seq.hip) ----
constexpr int kSeqMaxDeg = 8;
constexpr int kPipeThreads = 256;
constexpr int kPipeThreadsWide = 512;  // when a thread of 256 would hold 8 or more rows (1024 threads: 128 registers, spills: slower)
constexpr int kPipePairCap = 4096;     // FFM: entries^2 of the per-pair table (32 KB)

struct SeqKnobs {  // the table above; every int is kKnobUnset or the variable's atoi()
  int win = kKnobUnset, exact = kKnobUnset, nocond = kKnobUnset, w = kKnobUnset, par = kKnobUnset, trace = kKnobUnset;  // per call
  const char* trace_file = nullptr;                                                                                    // per call
  int pipe = kKnobUnset, stage = kKnobUnset;                                                                           // per process
};
inline SeqKnobs seq_knobs() {
  static const SeqKnobs once = [] {
    SeqKnobs k;
    k.pipe = mb_knob("NFM_SEQ_PIPE");
    k.stage = mb_knob("NFM_SEQ_STAGE");
    return k;
  }();
  SeqKnobs k = once;
  k.win = mb_knob("NFM_SEQ_WIN");
  k.exact = mb_knob("NFM_SEQ_WIN_EXACT");
  k.nocond = mb_knob("NFM_SEQ_WIN_NOCOND");
  k.w = mb_knob("NFM_SEQ_WIN_W");
  k.par = mb_knob("NFM_SEQ_WIN_PAR");
  k.trace = mb_knob("NFM_SEQ_WIN_TRACE");
  k.trace_file = getenv("NFM_SEQ_WIN_TRACE_FILE");
  return k;
}

struct SeqShape {  // what is fixed for one epoch call: the model as stored (ModelView), the dataset, the optimizer, the device
  int kind, degree, nb, kc, k, Kp, n_aug, fit_intercept;
  int64_t d, da, bs, rs;
  int m_cap;  // longest stored row + n_aug
  int64_t ns, nnz;
  int ada;    // AdaGrad
  int n_cu;
};

// ---------------------------------------------------------------------------------------------------------------------------
// the dependency window
// ---------------------------------------------------------------------------------------------------------------------------
enum WinReason {  // why a call is not supported, in the order the checks run
  WIN_OK = 0,
  WIN_OFF,     // NFM_SEQ_WIN=0
  WIN_KP,      // rows of more than 64 or fewer than 2 lanes
  WIN_SHAPE,   // augmented features, no blocks, an empty dataset where rows are slots, a degree beyond the workers'
  WIN_MAIL,    // term by term: more chain terms than a mailbox of kWinMaxNL loads holds
  WIN_LDS,     // the worker's LDS beyond a CU's, at the assumed worker count (kWinLdsSupportW / kWinLdsSupportWSlots)
  WIN_LIMITS,  // 2^32 entries, 2^31 features or samples
  WIN_CUS,     // fewer than 17 CUs
  WIN_SHORT    // fewer than 2048 samples, and NFM_SEQ_WIN is not 2
};

struct WinRoute {
  // A degree-2 FM of 65 ... 128 factors is ONE block of 128-double rows: too wide for the window's workers (rows of at most 64
  // factors).  The same table read as feature-major blocks of 64 -- row(b, j) = 2 j + b in units of 64 doubles, exactly
  // ModelView::row with bs = 1, rs = 2 -- is a two-block model of the same degree (common.h: kc), which the several-orders worker
  // takes as it is: no copy, no second layout.  The factors' sum is then formed block by block -- results within rounding of the
  // one-sample-in-flight kernel, not bit-equal: NFM_SEQ_WIN_EXACT=1 keeps such models on that kernel.
  int two_block;   // the view applies: everything below is of the model read that way (seq_window_view)
  int nb, Kp;      // blocks and lanes per row as the window sees them
  int supported, reason;  // WinReason
  int offered;     // supported, the snapshot pays, and the optimizer has not seen two launches abort
  // ---- the launch (set when supported) ----
  int no_cond;     // fitIntercept = false: no scalar chain, no conductor
  int one_term;    // the intercept is fitted: the one-term chain unless NFM_SEQ_WIN_EXACT
  int wk;          // WK_*
  int W, lgW, first_worker;  // workers (a power of two), workgroups ahead of them (the conductor: 1 or 0)
  int m_cap, lgKp;
  int terms, ch, FW;  // what a sample hands to the conductor's chain; the chain's chunk of terms; words per term-by-term mailbox
  int np, thr, near_r, par_min;
  size_t lds_worker, lds_cond, lds_bytes;  // lds_bytes: the larger of the two, at least kWinLdsFloor
  // elements of the buffers: mail = n_fwd + n_res words; ctl = n_ctl unsigned, then n_partial doubles (both zeroed per launch),
  // then two int64; fw = n_fw words of which the first n_fw_tags are zeroed per launch; scales in doubles (0: AdaGrad)
  size_t n_fwd, n_res, n_ctl, n_partial, n_fw, n_fw_tags, n_scales;
  int fits_cus;    // W > kWinDepth and W + first_worker <= n_cu
  int fits;        // ... and the LDS within a CU's at the real worker count.  0: the launcher answers NFM_WIN_FALLBACK
  const char* counter;
};

constexpr const char* kWinCounters[4] = {"seq_route_win_general", "seq_route_win_k64", "seq_route_win_ffm", "seq_route_win_fmx"};

namespace seq_detail {
inline int ffm_terms(int m_cap) { return m_cap + m_cap * (m_cap - 1) / 2; }
// the LDS a worker of kind `wk` asks for (seqwin_layout.h: the carve-up the kernels take their pointers from)
inline size_t worker_lds(int wk, int Kp, int nb, int k, int m_cap, bool ada, int W) {
  const WinShape s{Kp, win_lg(Kp), nb, k, m_cap, ada, W};
  return wk == WK_K64 ? win_k64_lds(s).total : wk == WK_GENERAL ? win_general_lds(s).total : win_slots_lds(s, wk == WK_FFM).total;
}
}  // namespace seq_detail

// does the two-blocks-of-64 view apply (the model as stored)
inline bool win_two_block(const SeqShape& S, const SeqKnobs& K) {
  if (K.exact != kKnobUnset && K.exact != 0) return false;
  if (!(S.kind == SEQ_KIND_FM && S.degree == 2 && S.n_aug == 0 && S.Kp == 2 * kWinLdsWave)) return false;
  // one block of 128-double rows (65 ... 128 factors), or a wide model of one order whose kc blocks of 128 lie feature-major
  // (api.hip: wide_rows): either way a feature's row is nb * 128 contiguous doubles = 2 nb blocks of 64
  const bool one_block = S.nb == 1 && S.kc == 1 && S.bs == S.da && S.rs == 1;
  const bool wide_rows = S.kc > 1 && S.nb == S.kc && S.bs == 1 && S.rs == S.nb;
  return one_block || wide_rows;
}

inline WinRoute win_route(const SeqShape& S, const SeqKnobs& K, int64_t fallbacks, size_t snap_bytes) {
  using namespace seq_detail;
  constexpr int kWave = kWinLdsWave;
  WinRoute r{};
  r.two_block = win_two_block(S, K);
  const int nb = r.nb = r.two_block ? 2 * S.nb : S.nb, Kp = r.Kp = r.two_block ? kWave : S.Kp, k = r.two_block ? kWave : S.k;
  const bool ada = S.ada != 0, ffm = S.kind == SEQ_KIND_FFM;
  const bool fmx = S.kind == SEQ_KIND_FM && (nb != 1 || S.degree != 2);  // several orders / degree >= 3
  // which flavour of the window the model gets
  r.no_cond = K.nocond != 0 && !S.fit_intercept;
  r.one_term = !r.no_cond && !(K.exact != kKnobUnset && K.exact != 0);
  r.counter = "";

  // ---- supported ----
  const int mode = K.win == kKnobUnset ? 1 : K.win;
  // a mailbox of one word per chain term bounds the row length only where the term-by-term conductor runs: not without a
  // conductor and not in the one-term window
  const bool term_mail = !(r.no_cond || r.one_term);
  const auto mail_full = [&](int terms) { return term_mail && kWinHdr + (terms + 63) / 64 * 64 > kWave * kWinMaxNL; };
  r.reason = [&] {
    if (mode == 0) return WIN_OFF;
    if (Kp > kWave || Kp < 2) return WIN_KP;
    if (ffm) {
      // field-aware: one chain term per entry and per pair of entries; all nFields rows of every feature in LDS
      if (S.n_aug != 0 || nb < 1 || S.m_cap < 1) return WIN_SHAPE;
      if (mail_full(ffm_terms(S.m_cap))) return WIN_MAIL;
      if (worker_lds(WK_FFM, Kp, nb, k, S.m_cap, ada, kWinLdsSupportWSlots) > kSeqLdsMax) return WIN_LDS;  // (AdaGrad keeps g_sum / g_norm of every slot beside the rows)
    } else if (fmx) {
      // several orders / degree >= 3: one chain term per entry and per order; the rows of every (entry, order) in LDS
      if (S.n_aug != 0 || nb < 1 || S.degree < 2 || S.degree > kWinLdsMaxDeg || S.m_cap < 1) return WIN_SHAPE;
      if (mail_full(S.m_cap + nb)) return WIN_MAIL;
      if (worker_lds(WK_FMX, Kp, nb, k, S.m_cap, ada, kWinLdsSupportWSlots) > kSeqLdsMax) return WIN_LDS;
    } else {
      if (S.kind != SEQ_KIND_FM || nb != 1 || S.degree != 2 || S.n_aug != 0) return WIN_SHAPE;
      if (mail_full(S.m_cap)) return WIN_MAIL;
      // (the general worker keeps the sample's rows in LDS)
      if (!(Kp == kWave && S.m_cap <= kWave) && worker_lds(WK_GENERAL, Kp, nb, k, S.m_cap, ada, kWinLdsSupportW) > kSeqLdsMax) return WIN_LDS;
    }
    if (S.nnz >= ((int64_t)1 << 32) || S.d >= ((int64_t)1 << 31) || S.ns >= ((int64_t)1 << 31)) return WIN_LIMITS;
    if (S.n_cu < 17) return WIN_CUS;  // the smallest window: 16 workers + the conductor, one CU each
    return mode == 2 || S.ns >= 2048 ? WIN_OK : WIN_SHORT;
  }();
  r.supported = r.reason == WIN_OK;
  // Is the call offered the window?  When the kernel takes the shape, the snapshot (one device-to-device copy at about 2 TB/s)
  // costs less than a quarter of the call (0.8 us per sample), and the optimizer has not seen two launches abort (CUs are
  // being held -- no more 1 s waits)
  const bool snap_pays = K.win == 2 || (double)S.ns * 0.8e-6 * 0.25 >= (double)snap_bytes / 2.0e12;
  r.offered = snap_pays && fallbacks < 2 && r.supported;
  if (!r.supported) return r;

  // ---- the launch ----
  const int m_cap = r.m_cap = S.m_cap < 1 ? 1 : S.m_cap;
  const bool k64 = !ffm && !fmx && Kp == kWave && m_cap <= kWave;  // the register-resident worker
  r.wk = ffm ? WK_FFM : fmx ? WK_FMX : k64 ? WK_K64 : WK_GENERAL;
  r.counter = kWinCounters[r.wk];
  // worker count: a power of two, one workgroup per CU with one CU left for the conductor.
  // With a conductor: 128 workers for the register-resident worker (64-factor rows: headline shape 2.36e6 -> 2.58e6 samples/s,
  // 2.8e6 with the chunk-parallel chain), 64 for the others (cfg2's shape: 2.36e6 against 2.2e6 at 128 -- its samples conflict
  // ten times as often, and every sample in flight is one more writer to wait for).  fitIntercept = false: no conductor, and
  // nothing but the features ties the samples -- twice the workers
  int W = r.no_cond || k64 ? 128 : 64;
  // rows of 64 factors without a conductor: a worker on EVERY CU (headline shape 5.8e6 -> 7.1e6 samples/s, AdaGrad 3.8e6 -> 5.9e6;
  // shorter rows conflict too often to gain) -- until a launch of this optimizer has aborted once: such a launch needs the
  // whole chip resident, and a tenant that holds a single CU would cost every call its 1 s limit.  (After a second abort
  // the window is not offered to this optimizer at all.)
  if (r.no_cond && k64 && fallbacks == 0) W = 256;
  if (K.w != kKnobUnset) W = K.w;
  int lgW = 4;
  while ((2 << lgW) <= W && lgW < (r.no_cond ? 8 : 7)) ++lgW;
  W = 1 << lgW;
  r.first_worker = r.no_cond ? 0 : 1;  // the conductor's CU (without a conductor no workgroup is launched for it)
  while (W + r.first_worker > S.n_cu && lgW > 4) W = 1 << --lgW;
  r.W = W;
  r.lgW = lgW;
  r.fits_cus = W > kWinDepth && W + r.first_worker <= S.n_cu;  // (n_cu >= 17 keeps other devices out)
  r.lgKp = win_lg(Kp);
  r.terms = ffm ? ffm_terms(m_cap) : fmx ? m_cap + nb : m_cap;
  r.ch = r.one_term || r.terms <= 32 ? 32 : 64;  // a mailbox holds MC = a multiple of it
  r.FW = r.one_term ? kWinHdr + 32 : kWinHdr + (r.terms + r.ch - 1) / r.ch * r.ch;  // (one-term mailboxes: kSumGran granules, see post_sum)
  // without a conductor the workers may run further apart (see the workers' run-ahead check): four buffer sets per worker
  // (measured: 2 / 4 / 8 sets 6.5e6 / 7.6e6 / 7.6e6 samples/s on the headline shape)
  r.np = r.no_cond ? 4 : 2;
  // without a conductor: how far back a dependency may lie and still take the recipe path (W), and how far apart the workers
  // may run (measured, headline shape at 256 workers / cfg2's at 128: recipes for dependencies up to W back 7.3e6 / 5.5e6
  // samples/s; up to 2W or 4W back 7.1e6 / 5.2e6: the longer reach only adds recipe stores)
  r.thr = r.np - 1;
  r.near_r = W;
  r.par_min = K.par == kKnobUnset ? 6 : K.par;  // (a parallel solve costs about as much as five or six samples of the serial loop)
  r.n_fwd = r.one_term ? (size_t)kSumGran * r.np * W : (size_t)W * r.np * r.FW;
  r.n_res = (size_t)W * r.np * kResWords;
  r.n_ctl = (size_t)W + 64;
  r.n_partial = 2 * ((size_t)W + 1);
  r.n_fw_tags = kFwSlot * r.np * (size_t)W;
  r.n_fw = (kFwSlot * r.np + 2 * kWave) * (size_t)W;  // + two scratch rows per worker
  r.n_scales = ada ? 0 : 2 * (size_t)S.ns;
  r.lds_worker = worker_lds(r.wk, Kp, nb, k, m_cap, ada, W);
  r.lds_cond = r.one_term ? sizeof(double) * (2 + 9 * (size_t)kSumRing) + sizeof(unsigned) * kSumRing
                          : sizeof(double) * 2 + sizeof(unsigned long long) * (size_t)kWinRing * r.FW;
  r.lds_bytes = r.lds_worker > r.lds_cond ? r.lds_worker : r.lds_cond;
  r.fits = r.fits_cus && r.lds_bytes <= kSeqLdsMax;  // (NFM_SEQ_WIN_W beyond what the support check assumed)
  if (r.lds_bytes < kWinLdsFloor) r.lds_bytes = kWinLdsFloor;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the one-workgroup kernels
// ---------------------------------------------------------------------------------------------------------------------------
// Where the per-sample table lives, beside the reduction buffer red[T]: in LDS when both fit a CU's, else in global scratch
struct SeqTable {
  int in_lds;
  size_t table_bytes, lds_bytes;  // lds_bytes: red[T], and the table where it is in LDS
};
inline SeqTable seq_sample_table(int T, size_t table_bytes) {
  const size_t both = sizeof(double) * (size_t)T + table_bytes;
  return both <= kSeqLdsMax ? SeqTable{1, table_bytes, both} : SeqTable{0, table_bytes, sizeof(double) * (size_t)T};
}

enum SeqStep { SEQ_PIPE, SEQ_STAGED, SEQ_PLAIN };
enum SeqRefusal { SEQ_OK = 0, SEQ_REFUSE_KP, SEQ_REFUSE_DEGREE };  // NFM_ERR_UNSUPPORTED: Kp > 1024; an FM's degree > kSeqMaxDeg

struct SeqOneWg {
  int refusal;  // SeqRefusal; nothing else is set when it is not SEQ_OK
  int step;     // SeqStep
  int m_cap;
  int T;        // Kp rounded up to whole wavefronts: the threads of k_sequential
  int threads;  // of the launch: T, or kPipeThreads / kPipeThreadsWide
  // the pipelined step: S = Kp rounded up to a power of two, rc = rows per thread on the rungs k_sequential_pipe is instantiated
  // for (1 ... 64 at kPipeThreads, 2 ... 16 at kPipeThreadsWide)
  int S, lgS, rc, split_terms;
  size_t lds_bytes;
  int table_in_lds;  // k_sequential's per-sample gradient [nb][m_cap][T] (1 under SEQ_PIPE as well: everything of a sample in LDS)
  size_t table_bytes;
  const char* counter;
};

inline SeqOneWg seq_one_wg_route(const SeqShape& M, const SeqKnobs& K) {
  SeqOneWg r{};
  r.counter = "";
  if (M.Kp > 1024) return r.refusal = SEQ_REFUSE_KP, r;
  const bool ffm = M.kind == SEQ_KIND_FFM;
  if (!(ffm || M.degree <= kSeqMaxDeg)) return r.refusal = SEQ_REFUSE_DEGREE, r;
  constexpr int kWave = kWinLdsWave;
  int T = ((M.Kp + kWave - 1) / kWave) * kWave;
  if (T < kWave) T = kWave;
  const int m_cap = M.m_cap < 1 ? 1 : M.m_cap;
  r.T = T;
  r.m_cap = m_cap;
  r.table_in_lds = 1;
  // The pipelined step (k_sequential_pipe): degree-2 FMs with one order and field-aware models; at most 256 factors and
  // 256 entries per row, at most 64 rows per thread, everything of a sample in LDS.
  if (K.pipe != 0 && (ffm || (M.nb == 1 && M.degree == 2)) && M.nb >= 1 && M.nb < 32768 && m_cap <= kPipeThreads) {
    int S = 2, lgS = 1;
    while (S < M.Kp) { S <<= 1; ++lgS; }
    const int nbk = ffm ? M.nb : 1;
    const int64_t slots = (int64_t)nbk * m_cap;
    int threads = kPipeThreads;
    int G = S <= threads ? threads / S : 0;
    int64_t rc = G > 0 ? (slots + G - 1) / G : (int64_t)1 << 30;
    if (G > 0 && rc >= 8 && (slots + 2 * G - 1) / (2 * G) <= 16) {  // 8 wavefronts: half of the rows per thread
      threads = kPipeThreadsWide;
      G *= 2;
      rc = (slots + G - 1) / G;
    }
    const size_t pair_doubles = ffm && (int64_t)m_cap * m_cap <= kPipePairCap ? (size_t)m_cap * m_cap : 0;
    // FM: the products of the per-factor sums are formed in parallel into one more [entries][S] table when it fits
    const size_t base_doubles = (size_t)threads + 2 * (size_t)slots * S + 7 * (size_t)m_cap + pair_doubles;
    const size_t tail_bytes = sizeof(int64_t) * 3 * (size_t)m_cap +
                              sizeof(int) * ((size_t)m_cap + (ffm ? 3 * (size_t)m_cap + nbk + (size_t)nbk * m_cap : 0));
    const int split_terms = !ffm && sizeof(double) * (base_doubles + (size_t)m_cap * S) + tail_bytes <= kSeqLdsMax ? 1 : 0;
    const size_t pipe_bytes = sizeof(double) * (base_doubles + (split_terms ? (size_t)m_cap * S : 0)) + tail_bytes;
    if (G >= 1 && rc <= 64 && pipe_bytes <= kSeqLdsMax) {
      const bool wide = threads == kPipeThreadsWide;  // rc <= 16
      int rung = wide ? 2 : 1;
      while (rung < rc) rung <<= 1;
      r.step = SEQ_PIPE;
      r.threads = threads, r.S = S, r.lgS = lgS, r.rc = rung, r.split_terms = split_terms, r.lds_bytes = pipe_bytes;
      r.counter = wide ? "seq_route_pipe_wide" : "seq_route_pipe";
      return r;
    }
  }
  // the per-sample gradient [nb][m_cap][T]: in LDS, or in global scratch when it does not fit (long rows, many blocks)
  const size_t n_da = (size_t)(M.nb > 0 ? M.nb : 1) * m_cap * T;
  const SeqTable tab = seq_sample_table(T, sizeof(double) * n_da);
  r.threads = T;
  r.table_in_lds = tab.in_lds, r.table_bytes = tab.table_bytes, r.lds_bytes = tab.lds_bytes;
  // staged step (entries and parameter values in LDS) when the extra [nb][m_cap][T] + 2 [m_cap] doubles fit
  const size_t staged_bytes = tab.lds_bytes + sizeof(double) * (n_da + 3 * (size_t)m_cap);
  if (!ffm && tab.in_lds && K.stage != 0 && M.nb > 0 && staged_bytes <= kSeqLdsMax) {
    r.step = SEQ_STAGED;
    r.lds_bytes = staged_bytes;
    r.counter = "seq_route_staged";
  } else {
    r.step = SEQ_PLAIN;
    r.counter = tab.in_lds ? "seq_route_plain" : "seq_route_plain_scratch";
  }
  return r;
}

}  // namespace nfm
