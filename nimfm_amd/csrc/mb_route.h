// nimfm_amd/csrc/mb_route.h -- which kernels a mini-batch of NFM_MODE_MINIBATCH (FactorizationMachine) takes, on which grids,
// decided once per batch as a pure function: mb_route(shape, knobs, batch).  run_batches (mb_fm_kernels.h) builds the argument
// structs from the answer and launches; mb_fm_epoch (mb_fm.hip) sizes the work buffers from the same formulas
// (mb_work_bounds).  Plain C++17, no HIP header: tests/cpp/mb_route_test.cpp holds it against the restatement of
// tests/row_slot_cases.py and tests/mb_route_cases.py with g++ alone.  Why each choice is what it is: DESIGN.md section 7 and
// the comments at the kernels (mb_fm_kernels.h).
//
// The environment knobs of the driver, all read by mb_knobs() and nowhere else:
//   knob                   read          what it overrides (unset = the default)
//   NFM_TU                 per call      records / A rows requested together per feature in the column walk: 2; 1 and 4 are the
//                                        tuning variants of k_col_phase (never strided, not instantiated for MBPSGD)
//   NFM_COL_LONG           per call      0: never k_col_long; 1: every batch the pipelined walk could take; unset: a capped batch
//                                        at L = 32 whose features are touched kColLongMean times or more on average
//   NFM_COL_LONG_COMPACT   per call      0: k_col_long never forms SGD's step sizes itself (and nothing is staged)
//   NFM_STAGE_DL           per call      0: never k_stage_dl; otherwise with k_col_long's compact variant
//   NFM_STAGE_W            per call      0: never stage w; 1: every batch whose row phase is MODE 1; unset: those that take k_col_long
//   NFM_STAGE_W_PASSES     per call      0: feature slices (k_stage_w); n: n passes over the entry range (k_stage_w_ranges);
//                                        unset: kStagePasses where every row ascends, slices otherwise
//   NFM_COL_GRID           per call      n > 0: at most n feature workgroups, strided (tests: small shapes reach the strided walks)
//   NFM_STREAM             per process   0 | 1: non-temporal row stores off | on; unset: singles and tables beyond kStreamTableBytes
//   NFM_SINGLES_KERNEL     per process   1: the singles in a kernel of their own (k_singles), not in the row phase
//   NFM_HELD               per process   0: no held entries (row MODE 0 everywhere)
//   NFM_NQ                 per process   0: no register-resident rows (row MODE 2 / 4 become 1)
//   NFM_COL_PIPE           per process   0: no software-pipelined walks (k_col_sparse, k_col_long)
//   NFM_COL_WG             per process   workgroups per CU of a capped column grid; unset: the strided kernel's occupancy
//   NFM_COL_CAP_SETS       per process   resident sets beyond which the column grid is capped: 4
//   NFM_ADA2               per process   0: no k_row_phase_ada2
// "per call": at every epoch call (tests flip them inside one process); "per process": at the first one.
// NFM_SPLIT (the row slots) is read by choose_split (lane_map.h), which decisionFunction shares.
#pragma once
#include <limits.h>

#include <algorithm>

#include "lane_map.h"

namespace nfm {

enum { MB_SGD = 0, MB_ADAGRAD = 1, MB_PSGD = 2 };  // = OPT_SGD, OPT_ADAGRAD, OPT_PSGD (opt_views.h; asserted in mb_fm_kernels.h)

// mean touches per column-phase feature from which a batch takes k_col_long: the headline shape's batch sweep
// (profiles/r06a_col_long_batch_sweep.txt) has it slower than k_col_sparse at 2.4 (batch 32768) and faster from 4.3 (65536) on.
// Measured at k = 64 (L = 32) only, so only that width switches by itself.
constexpr double kColLongMean = 4.0;
constexpr int kStagePasses = 4;  // the default for datasets whose rows ascend (measured: DESIGN.md section 7, round 8)
constexpr int64_t kStageSliceBytes = (int64_t)2 << 20;  // of the 4 MB L2: the slice's weights beside the index and output streams
// tables far beyond the 256 MB Infinity Cache, batches that visit most rows once: their rows are streamed (st_nt / ld_nt)
constexpr uint64_t kStreamTableBytes = (uint64_t)384 << 20;
constexpr int kColCapSets = 4;
constexpr int kMaxBlocksPerCu = 8;  // workgroups of kLaneBlock lanes a CU holds at most (8 wavefronts per SIMD): bounds any occupancy

// E: entries a lane holds in the held row modes (k_row_phase MODE 1 - 4) at L lanes per row and s row slots per sample;
// 0 = no held mode for this lane mapping.  Rows of up to held_capacity entries are taken whole.
constexpr int held_entries(int L, int s) {
  const int lps = L * s;
  return lps >= kLaneWave ? 1 : (lps >= 8 ? (kLaneWave / lps > 4 ? 4 : kLaneWave / lps) : 0);
}
constexpr int held_capacity(int L, int s) { return held_entries(L, s) * L * s; }
constexpr bool held_rows_fit_a_wave() {  // what the staged weights' buffer is sized by (mb_work_bounds)
  for (int L = 1; L <= kLaneWave; L <<= 1)
    for (int s = 1; L * s <= kLaneWave; s <<= 1)
      if (held_capacity(L, s) > kLaneWave) return false;
  return true;
}
static_assert(held_rows_fit_a_wave(), "a held row is at most kLaneWave entries");

// the row slots k_row_phase is instantiated for: choose_split's answer on the rungs 16, 8, 4, 2, 1, within the R = 64 / L a wavefront has
constexpr int row_slots(int split, int R) {
  return (R >= 16 && split >= 16) ? 16 : (R >= 8 && split >= 8) ? 8 : (R >= 4 && split >= 4) ? 4 : (R >= 2 && split >= 2) ? 2 : 1;
}

constexpr int kKnobUnset = INT_MIN;
struct MbKnobs {  // the table above; every field is kKnobUnset or the variable's atoi()
  int tu = kKnobUnset, col_long = kKnobUnset, col_long_compact = kKnobUnset, stage_dl = kKnobUnset, stage_w = kKnobUnset,
      stage_w_passes = kKnobUnset, col_grid = kKnobUnset;  // per call
  int stream = kKnobUnset, singles_kernel = kKnobUnset, held = kKnobUnset, nq = kKnobUnset, col_pipe = kKnobUnset,
      col_wg = kKnobUnset, col_cap_sets = kKnobUnset, ada2 = kKnobUnset;  // per process
};
inline int mb_knob(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : kKnobUnset;
}
inline MbKnobs mb_knobs() {
  static const MbKnobs once = [] {
    MbKnobs k;
    k.stream = mb_knob("NFM_STREAM");
    k.singles_kernel = mb_knob("NFM_SINGLES_KERNEL");
    k.held = mb_knob("NFM_HELD");
    k.nq = mb_knob("NFM_NQ");
    k.col_pipe = mb_knob("NFM_COL_PIPE");
    k.col_wg = mb_knob("NFM_COL_WG");
    k.col_cap_sets = mb_knob("NFM_COL_CAP_SETS");
    k.ada2 = mb_knob("NFM_ADA2");
    return k;
  }();
  MbKnobs k = once;
  k.tu = mb_knob("NFM_TU");
  k.col_long = mb_knob("NFM_COL_LONG");
  k.col_long_compact = mb_knob("NFM_COL_LONG_COMPACT");
  k.stage_dl = mb_knob("NFM_STAGE_DL");
  k.stage_w = mb_knob("NFM_STAGE_W");
  k.stage_w_passes = mb_knob("NFM_STAGE_W_PASSES");
  k.col_grid = mb_knob("NFM_COL_GRID");
  return k;
}

struct MbShape {  // what is fixed for one epoch call
  int L, opt, gen;  // lanes per row; MB_SGD / MB_ADAGRAD / MB_PSGD; anything but one order of degree 2
  int nb, n_aug, fit_linear;
  int64_t d;
  int max_row;     // longest stored row
  double avg_row;  // mean entries per row, augmented
  int n_cu;
  int use_singles, first_singleton;  // of the plan
  int rows_ascend;                   // every row of the dataset ascends
  uint64_t table_bytes;              // parameter (and state) tables
  int compact_sched;  // SGD's schedule takes no pow(): k_col_long can form the step sizes itself (always 1 for the others)
  int col_occ;        // workgroups per CU of the strided column kernel of this instantiation (queried by the caller)
};

struct MbBatch {  // what the plan says about one mini-batch
  int64_t b;      // its index in the plan
  int len;        // samples
  int64_t uniq, touches, heavy, segs;  // column-phase features and their touches; heavy features and their segments
};

enum MbRowKernel { MB_ROW_PHASE, MB_ROW_ADA2 };
enum MbStageW { MB_W_GATHER, MB_W_SLICES, MB_W_RANGES };  // the row phase gathers w | k_stage_w | k_stage_w_ranges
enum MbColKernel { MB_COL_PHASE, MB_COL_STRIDED, MB_COL_SPARSE, MB_COL_LONG, MB_COL_LONG_COMPACT, MB_COL_TU1, MB_COL_TU4 };

struct MbRoute {
  int use_stored;  // the batch reads the stored parameters (MBPSGD; AdaGrad's first step)
  // row phase: k_row_phase<L, slots, .., mode, sing> or k_row_phase_ada2<.., stream_rows> on nA workgroups
  int row_kernel, slots, mode, sing, stream_rows, nA;
  int singles_in_row, singles_in_col, nS;  // nS: workgroups of k_singles
  // the linear weights in sample order, stride w_cap: w_parts slices of w_slice features or w_parts passes, w_wg workgroups each
  int stage_w, w_cap, w_parts, w_wg;
  int64_t w_slice;
  int bad_passes;  // stage_w with an NFM_STAGE_W_PASSES that is not 0 or a power of two up to w_cap: nothing may be launched
  int stage_dl, dl_grid;
  int col_kernel, nB;  // nB includes the closing workgroup
  int nsb, nH;         // heavy features: k_heavy_partial / k_heavy_apply workgroups, 0 = none
};

inline const char* mb_row_counter(const MbRoute& r) {
  static const char* const m[] = {"route_row_m0", "route_row_m1", "route_row_m2", "route_row_m3", "route_row_m4"};
  return r.row_kernel == MB_ROW_ADA2 ? "route_row_ada2" : m[r.mode];
}
inline const char* mb_col_counter(const MbRoute& r) {
  static const char* const c[] = {"route_col_phase", "route_col_strided", "route_col_sparse", "route_col_long", "route_col_long_compact",
                                  "route_col_tu1", "route_col_tu4"};
  return c[r.col_kernel];
}

namespace route_detail {
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool off(int knob) { return knob == 0; }  // "NAME=0"; kKnobUnset is not 0
inline int or_default(int knob, int dflt) { return knob == kKnobUnset ? dflt : knob; }

// workgroups of the row phase over len samples
inline int row_blocks(int len, int L, int slots) { return (int)ceil_div(len, kLaneWavesPerBlock * (kLaneWave / (L * slots))); }
inline int ada2_blocks(int len) { return (len + 1) / 2; }  // two wavefronts per sample
inline int sample_blocks(int64_t n) { return (int)ceil_div(n, kLaneWavesPerBlock); }  // one wavefront per sample / heavy feature
inline int feature_blocks(int64_t n, int L) { return (int)ceil_div(n, kLaneWavesPerBlock * (kLaneWave / L)); }  // L lanes per feature

inline bool singles_in_row(const MbShape& S, const MbKnobs& K) {
  return !S.gen && S.use_singles && !(K.singles_kernel != kKnobUnset && K.singles_kernel != 0);
}
inline bool ada2_shape(const MbShape& S, const MbKnobs& K) {
  return S.opt == MB_ADAGRAD && !S.gen && S.L == 32 && !off(K.ada2) && singles_in_row(S, K) && S.max_row + S.n_aug <= 64;
}
// the software-pipelined walks: one order of degree 2, SGD / AdaGrad
inline bool col_pipe(const MbShape& S, const MbKnobs& K) { return !off(K.col_pipe) && !S.gen && S.nb == 1 && S.opt != MB_PSGD; }
// can any batch of this call take k_col_long
inline bool may_col_long(const MbShape& S, const MbKnobs& K) {
  return col_pipe(S, K) && or_default(K.tu, 2) == 2 && !off(K.col_long) && (K.col_long != kKnobUnset || S.L == 32);
}
inline bool compact(const MbShape& S, const MbKnobs& K) { return !off(K.col_long_compact) && S.compact_sched; }
// row-phase mode (k_row_phase) at `slots`: 2 = held entries + register-resident rows (SGD, one sample per wavefront, a batch
// with singles), 1 = held entries, 3 = held entries in chunks (rows longer than the held capacity), 0 = streamed (degree-1
// models: linear term only; samples spread over fewer than 8 lanes)
inline int row_mode(const MbShape& S, const MbKnobs& K, int slots) {
  const int cap = held_capacity(S.L, slots);
  if (off(K.held) || cap == 0 || S.nb == 0) return 0;
  if (S.max_row + S.n_aug > cap) return 3;
  if (!S.gen && !off(K.nq) && S.opt == MB_SGD && singles_in_row(S, K) && S.L * slots == kLaneWave) return 2;
  return 1;
}
// can a batch at `slots` row slots have its linear weights staged (SGD with a fitted linear term, rows within the held capacity;
// with the schedules k_col_long's compact variant takes: what was measured)
inline bool may_stage_w(const MbShape& S, const MbKnobs& K, int slots) {
  return S.opt == MB_SGD && !S.gen && S.fit_linear && row_mode(S, K, slots) == 1 && !off(K.stage_w) && compact(S, K) &&
         (K.stage_w != kKnobUnset || may_col_long(S, K));
}
// Feature workgroups of the column phase, without the closing one.  Beyond cap_sets resident sets the grid is capped at ONE
// resident set (col_wg workgroups per CU) and the workgroups stride over the features; NFM_COL_GRID caps at its own count.
inline int col_blocks(const MbShape& S, const MbKnobs& K, int64_t uniq, bool* capped) {
  int nB = feature_blocks(uniq, S.L);
  const int col_wg = or_default(K.col_wg, S.col_occ), grid = or_default(K.col_grid, 0);
  *capped = or_default(K.tu, 2) == 2 &&
            ((col_wg > 0 && nB > (int64_t)or_default(K.col_cap_sets, kColCapSets) * S.n_cu * col_wg) || (grid > 0 && nB > grid));
  if (*capped) nB = grid > 0 ? std::min(nB, grid) : S.n_cu * col_wg;
  return nB;
}
}  // namespace route_detail

inline MbRoute mb_route(const MbShape& S, const MbKnobs& K, const MbBatch& B) {
  using namespace route_detail;
  MbRoute r{};
  const int tu = or_default(K.tu, 2);
  // MBPSGD: the forward pass is AdaGrad's row phase reading the stored parameters; AdaGrad's very first step does the same
  r.use_stored = S.opt == MB_PSGD || (S.opt == MB_ADAGRAD && S.first_singleton && B.b == 0);
  const bool have_singles = !S.gen && S.use_singles;
  r.singles_in_row = singles_in_row(S, K);
  r.singles_in_col = have_singles && !r.singles_in_row;
  r.stream_rows = K.stream != kKnobUnset && K.stream >= 0 ? K.stream != 0 : (have_singles && S.table_bytes > kStreamTableBytes);
  // row phase
  r.slots = row_slots(choose_split(S.L, B.len, S.avg_row, S.n_cu), kLaneWave / S.L);
  const int mode = row_mode(S, K, r.slots);
  if (ada2_shape(S, K) && !r.use_stored) {  // AdaGrad, 32 < k <= 64, rows of at most 64 entries, singles in the row phase
    r.row_kernel = MB_ROW_ADA2;
    r.slots = 2;
    r.nA = ada2_blocks(B.len);
  } else {
    r.row_kernel = MB_ROW_PHASE;
    r.mode = mode == 2 && r.stream_rows ? 4 : mode;  // MODE 4: MODE 2 with streamed stores
    r.sing = mode == 0 && r.singles_in_row;
    r.nA = row_blocks(B.len, S.L, r.slots);
  }
  r.nS = r.singles_in_col ? sample_blocks(B.len) : 0;
  // column phase: which kernel the batch takes is known before its row phase (the staging goes with k_col_long)
  bool capped;
  r.nB = col_blocks(S, K, B.uniq, &capped) + 1;
  const bool col_long = may_col_long(S, K) && (K.col_long != kKnobUnset || (capped && (double)B.touches >= kColLongMean * (double)B.uniq));
  const bool cmp = compact(S, K);
  if (tu == 1 && S.opt != MB_PSGD) r.col_kernel = MB_COL_TU1;
  else if (tu == 4 && S.opt != MB_PSGD) r.col_kernel = MB_COL_TU4;
  else if (col_long) r.col_kernel = cmp ? MB_COL_LONG_COMPACT : MB_COL_LONG;
  else if (capped) r.col_kernel = col_pipe(S, K) ? MB_COL_SPARSE : MB_COL_STRIDED;
  else r.col_kernel = MB_COL_PHASE;
  // the batch's dL in touch order for k_col_long<.., COMPACT> (the other column kernels read what they read)
  r.stage_dl = col_long && cmp && !off(K.stage_dl) && B.touches > 0;
  if (r.stage_dl) r.dl_grid = (int)std::min<int64_t>(ceil_div(B.touches, 4 * kLaneBlock), (int64_t)S.n_cu * 32);
  // the linear weights in sample order for k_row_phase<.., MODE 1>: where the column phase is k_col_long, the row phase's w
  // gather is a fifth of its requests beyond L2
  r.w_cap = held_capacity(S.L, r.slots);
  if (may_stage_w(S, K, r.slots) && (K.stage_w != kKnobUnset || col_long)) {
    const int passes = or_default(K.stage_w_passes, S.rows_ascend ? kStagePasses : 0);
    int64_t spw;  // samples per wavefront step
    if (passes != 0) {
      r.stage_w = MB_W_RANGES;
      r.w_parts = passes;
      if (!(passes > 0 && passes <= r.w_cap && (passes & (passes - 1)) == 0)) {
        r.bad_passes = 1;
        return r;
      }
      spw = kLaneWave / (r.w_cap / passes);
    } else {
      r.stage_w = MB_W_SLICES;
      r.w_parts = (int)std::max<int64_t>(1, ceil_div((int64_t)sizeof(double) * S.d, kStageSliceBytes));
      r.w_slice = ceil_div(S.d, r.w_parts);
      spw = kLaneWave / r.w_cap;
    }
    r.w_wg = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(ceil_div(B.len, spw), kLaneWavesPerBlock), (int64_t)S.n_cu * 8));
  }
  if (S.nb > 0 && B.heavy > 0) {
    r.nsb = feature_blocks(B.segs, S.L);
    r.nH = sample_blocks(B.heavy);
  }
  return r;
}

// Element counts of the work buffers the routes of one epoch call can ask for, from the plan's maxima: the largest batch, the
// most column-phase features, touches and heavy features of one batch.
struct MbBounds {
  int64_t partsA;  // PartA records: one per row-phase workgroup
  int64_t partsB;  // doubles, BOTH halves: one per workgroup of k_singles, the column phase and k_heavy_apply, per half
  int64_t dLt;     // doubles of the staged dL stream, 0 = no batch can be staged
  int64_t Wt;      // doubles of the staged linear weights, 0 = no batch can be staged
};
inline MbBounds mb_work_bounds(const MbShape& S, const MbKnobs& K, int64_t max_batch, int64_t max_unique, int64_t max_touch, int64_t max_heavy) {
  using namespace route_detail;
  MbBounds o{};
  // the fewest samples a row-phase workgroup takes: kLaneWavesPerBlock at one sample per wavefront, 2 in k_row_phase_ada2
  o.partsA = std::max(1, ada2_shape(S, K) ? ada2_blocks((int)max_batch) : sample_blocks(max_batch));
  // a capped column grid is below the uncapped one unless NFM_COL_CAP_SETS is below 1 (tuning): then one resident set
  const int col_wg = or_default(K.col_wg, S.col_occ);
  int64_t nB = feature_blocks(max_unique, S.L);
  if (col_wg > 0 && or_default(K.col_cap_sets, kColCapSets) < 1) nB = std::max<int64_t>(nB, (int64_t)S.n_cu * col_wg);
  const bool singles_col = !S.gen && S.use_singles && !singles_in_row(S, K);
  o.partsB = 2 * ((singles_col ? sample_blocks(max_batch) : 0) + nB + 1 + (S.nb > 0 ? sample_blocks(max_heavy) : 0));
  o.dLt = may_col_long(S, K) && compact(S, K) && !off(K.stage_dl) ? max_touch : 0;
  // every held capacity is at most kLaneWave entries; which of them a batch has depends on its own length (choose_split)
  bool w = false;
  for (int s = 1; s <= 16 && s <= kLaneWave / S.L; s <<= 1) w = w || may_stage_w(S, K, s);
  o.Wt = w ? std::max<int64_t>(max_batch, 1) * kLaneWave : 0;
  return o;
}

}  // namespace nfm
