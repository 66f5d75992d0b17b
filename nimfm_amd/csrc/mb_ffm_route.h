// nimfm_amd/csrc/mb_ffm_route.h -- which kernels a mini-batch of NFM_MODE_MINIBATCH (FieldAwareFactorizationMachine) takes, on
// which grids and with how much LDS, as pure functions: ffm_row_kernel(shape, knobs) once per epoch call, ffm_route(shape, knobs,
// row, batch) once per batch.  run_ffm (mb_ffm.hip) builds the argument structs from the answers and launches; mb_ffm_epoch sizes
// the work buffers from the same formulas (ffm_work_bounds); the launch's LDS bytes come from ffm_row_lds, the layout
// k_ffm_row_phase_lds carves (the kernel keeps its own lines of it: profiles/mb_ffm_route_resources.txt).  Plain C++17, no HIP
// header: tests/cpp/mb_ffm_route_test.cpp holds it against the restatement of tests/ffm_kernel_cases.py with g++ alone.  Why each
// choice is what it is: the comments at the kernels (mb_ffm.hip).
//
// The environment knobs of the driver, both read by ffm_knobs() and nowhere else:
//   knob              read          what it overrides (unset = the default)
//   NFM_FFM_LDS       per process   0: never k_ffm_row_phase_lds (every batch takes the generic row kernel)
//   NFM_FFM_REFRESH   per process   0: never k_ffm_refresh; 2: in front of every AdaGrad batch but the stored first step; unset (or
//                                   anything else): in front of those whose touches are kRefreshMean times their features or more
#pragma once
#include <stddef.h>

#include "mb_route.h"  // kKnobUnset, mb_knob, MB_SGD / MB_ADAGRAD, the workgroup counts of route_detail

namespace nfm {

// of the 160 KiB of a CU: what the row kernel's workgroup may ask for (above kFfmLdsDefault the launch needs
// hipFuncAttributeMaxDynamicSharedMemorySize raised)
constexpr size_t kFfmLdsShare = 150 * 1024;
constexpr size_t kFfmLdsDefault = 64 * 1024;
// k_ffm_refresh is worth its pass over the batch's (feature, field) units when a unit is read by several samples of the batch
// (cfg4: 5.2 touches per feature, 4.8e7 -> 5.1e7 samples/s; the 39-field shape: 2.7, 1.3e7 -> 1.16e7: not there)
constexpr double kRefreshMean = 4.0;

struct FfmKnobs {  // the table above; every field is kKnobUnset or the variable's atoi()
  int lds = kKnobUnset, refresh = kKnobUnset;
};
inline FfmKnobs ffm_knobs() {
  static const FfmKnobs once = [] {
    FfmKnobs k;
    k.lds = mb_knob("NFM_FFM_LDS");
    k.refresh = mb_knob("NFM_FFM_REFRESH");
    return k;
  }();
  return once;
}

struct FfmShape {  // what is fixed for one epoch call
  int L, opt;      // lanes per row; MB_SGD / MB_ADAGRAD
  int nb, Kp;      // fields; padded components (2 L)
  int max_row;     // longest stored row of the dataset
  int first_singleton;  // of the plan
};

// Per-sample LDS of k_ffm_row_phase_lds for rows of up to m_cap entries (byte offsets from the sample's base):
// rows [m_cap * F][Kp] doubles, fmask [F] u64, xs [m_cap] doubles, js and fs [m_cap] ints; per_wave: all of it, rounded up to 16
struct FfmRowLds {
  size_t rows, fmask, xs, js, fs, per_wave;
};
constexpr FfmRowLds ffm_row_lds(int m_cap, int F, int Kp) {
  const size_t fmask = (size_t)m_cap * F * Kp * 8, xs = fmask + (size_t)F * 8;
  const size_t js = xs + (size_t)m_cap * 8, fs = js + (size_t)m_cap * 4;
  return FfmRowLds{0, fmask, xs, js, fs, (fs + (size_t)m_cap * 4 + 15) / 16 * 16};
}

enum FfmRowKernel { FFM_ROW_GENERIC, FFM_ROW_LDS, FFM_ROW_COOP };  // k_ffm_row_phase | k_ffm_row_phase_lds<.., 4, false> | <.., 4, true>
constexpr const char* kFfmRowBigCounter = "ffm_row_lds_big";

struct FfmRow {
  int kernel, m_cap;  // m_cap: the kernel's row capacity, max_row but at least 1
  size_t lds_bytes;   // dynamic LDS of the launch
  int wpb;            // samples per workgroup: 4 (one per wavefront), 1 under FFM_ROW_COOP (the workgroup's wavefronts share it)
  int raise_lds_limit;  // lds_bytes > kFfmLdsDefault: counted under kFfmRowBigCounter as well
  const char* counter;
};

// LDS-resident neighbourhood: rows of at most 64 entries, at most 64 fields, m_cap * F parameter rows that fit a quarter of
// the LDS share (four samples per workgroup) or the share itself (one); NFM_FFM_LDS=0 and everything else: the generic kernel
inline FfmRow ffm_row_kernel(const FfmShape& S, const FfmKnobs& K) {
  FfmRow r{FFM_ROW_GENERIC, S.max_row > 1 ? S.max_row : 1, 0, kLaneWavesPerBlock, 0, "ffm_row_generic"};
  if (K.lds != 0 && S.max_row <= kLaneWave && S.nb <= kLaneWave) {
    const size_t per_wave = ffm_row_lds(r.m_cap, S.nb, S.Kp).per_wave;
    if (per_wave * 4 <= kFfmLdsShare)
      r.kernel = FFM_ROW_LDS, r.lds_bytes = per_wave * 4, r.counter = "ffm_row_lds";
    else if (per_wave <= kFfmLdsShare)
      r.kernel = FFM_ROW_COOP, r.lds_bytes = per_wave, r.wpb = 1, r.counter = "ffm_row_coop";
  }
  r.raise_lds_limit = r.lds_bytes > kFfmLdsDefault;
  return r;
}

struct FfmBatch {  // what the plan says about one mini-batch
  int64_t b;       // its index in the plan
  int len;         // samples
  int64_t uniq, touches, heavy, segs;  // unique features and all touches of the batch; heavy features and their segments
};

struct FfmRoute {
  int refresh;     // k_ffm_refresh in front of the batch
  int use_stored;  // row and column phase take the parameters as stored: AdaGrad's first step, and after a refresh
  int nA;          // row phase
  int nR, nB;      // k_ffm_refresh (0 = none); k_ffm_col_phase, the closing workgroup included
  int nsb, nH;     // heavy features: k_ffm_heavy_partial / k_ffm_heavy_apply workgroups, 0 = none
  // one viol partial per workgroup in the batch's half of partsB: the refresh pass, the column phase, k_ffm_heavy_apply
  int off_refresh, off_col, off_heavy;
  int n_parts;  // all of them: what the next batch's closing workgroup adds up
};

inline FfmRoute ffm_route(const FfmShape& S, const FfmKnobs& K, const FfmRow& row, const FfmBatch& B) {
  using namespace route_detail;
  FfmRoute r{};
  const bool first_stored = S.opt == MB_ADAGRAD && S.first_singleton && B.b == 0;
  r.refresh = S.opt == MB_ADAGRAD && !first_stored && K.refresh != 0 &&
              (K.refresh == 2 || (double)B.touches >= kRefreshMean * (double)B.uniq);
  r.use_stored = first_stored || r.refresh;
  r.nA = (int)ceil_div(B.len, row.wpb);
  const int units = feature_blocks(B.uniq * S.nb, S.L);  // a unit = (feature, field), L lanes each
  r.nR = r.refresh ? std::max(1, units) : 0;  // (the intercept is workgroup 0's)
  r.nB = units + 1;
  if (B.heavy > 0) {
    r.nsb = feature_blocks(B.segs * S.nb, S.L);  // L lanes per (segment, field)
    r.nH = sample_blocks(B.heavy * S.nb);        // one wavefront per (heavy feature, field)
  }
  r.off_refresh = 0, r.off_col = r.nR, r.off_heavy = r.nR + r.nB;
  r.n_parts = r.nR + r.nB + r.nH;
  return r;
}

// Element counts of the work buffers the routes of one epoch call can ask for, from the plan's maxima: the largest batch, the
// most unique features, touches, heavy features and heavy segments of one batch.
struct FfmBounds {
  int64_t contrib;  // doubles: [touches][F][Kp]
  int64_t rec;      // SampleRec records: one per sample
  int64_t partsA;   // PartA records: one per row-phase workgroup
  int64_t partsB;   // doubles, BOTH halves: FfmRoute::n_parts per half
  int64_t hpart;    // doubles: [segments][F][2 Kp + 4]
};
inline FfmBounds ffm_work_bounds(const FfmShape& S, const FfmRow& row, int64_t max_batch, int64_t max_unique, int64_t max_touch,
                                 int64_t max_heavy, int64_t max_segs) {
  using namespace route_detail;
  FfmBounds o{};
  o.contrib = std::max<int64_t>(max_touch, 1) * S.nb * S.Kp;
  o.rec = std::max<int64_t>(max_batch, 1);
  o.partsA = std::max<int64_t>(ceil_div(max_batch, row.wpb), 1);
  const int64_t units = feature_blocks(max_unique * S.nb, S.L);
  o.partsB = 2 * ((S.opt == MB_ADAGRAD ? std::max<int64_t>(1, units) : 0) + units + 1 + sample_blocks(max_heavy * S.nb));
  o.hpart = std::max<int64_t>(max_segs, 1) * S.nb * (2 * S.Kp + 4);
  return o;
}

}  // namespace nfm
