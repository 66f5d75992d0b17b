// nimfm_amd/csrc/plan_route.h -- who builds a batch plan, and in which instantiation, decided as pure functions.  plan.hip has
// three builders that promise the same arrays (plan.h); plan_build tries them in this order:
//   1. the column-major twin (Plan::kByTwin)   twin_route(shape, knobs, T); after its count pass, twin_clashed(clash, touches, T)
//   2. bucketing (Plan::kBySeg)                seg_route(shape, knobs, T); after its count pass, seg_gives_up(largest cell)
//   3. the device-wide sort (Plan::kBySort)    always possible; plan_key() gives its key
// A twin that clashed leaves the build to 2 and 3, bucketing that gave up to 3.  Plain C++17, no HIP header:
// tests/cpp/plan_route_test.cpp holds every function against the restatement of tests/plan_route_cases.py and against a copy of
// the lines they replaced, with g++ alone.  DESIGN.md, "The route of a plan build", says where each threshold came from.
//
// The environment knobs of the build, all read by plan_knobs() and nowhere else:
//   knob           read        what it overrides (unset = the default)
//   NFM_PLAN_CSC   per build   0: never the column-major twin
//   NFM_PLAN_KEY   per build   0: the twin takes positions from the table of the inverse order, also for device-drawn orders
//   NFM_PLAN_SEG   per build   0: never bucketing
//   NFM_SEG_FL     per build   8 ... 12: the bucket width 2^fl, whatever the shape says; anything else is ignored
//   NFM_SEG_S      per build   > 0: samples per chunk workgroup; unset or <= 0: 256
//   NFM_SEG_XCD    per build   0: the plain workgroup order (workgroup = batch * per_batch + part), not one XCD per batch
// "per build": at every plan_build (the tests switch them inside one process).
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace nfm {

// the wavefront and the workgroup the rungs below count in (plan.hip asserts them against common.h's kWave and kBlock)
constexpr int kPlanWave = 64;
constexpr int kPlanBlock = 256;

// ---- the twin's constants (plan.hip: "Plans from the column-major twin of the data") ----
constexpr int kCscMaxCol = 1024;      // longest column the ranking kernel takes (16 entries per lane)
constexpr int kCscMaxBatches = 512;   // per-wavefront LDS: k_csc_fill 256 NE + 2 x 512 + 2 ints (NE = 16: 20.5 KB, two wavefronts per workgroup), k_csc_count 4 x 512 ints
// one wavefront of k_csc_count per kCntGroup consecutive features: the counts of the group leave as runs of kCntGroup
// consecutive ints per batch
constexpr int kCntGroup = 4;
constexpr size_t kCscFillLds = 48 * 1024;  // the most a workgroup of k_csc_fill asks for (twin_fill)
constexpr double kCscMaxCells = 268435456.0;  // 2^28 (batch, feature) cells: the twin's count table and its scan hold one entry per cell
constexpr double kCscMinFill = 0.5;           // dense batches: at least half of the (batch, feature) cells' worth of touches

// ---- bucketing's constants (plan.hip: "plans by bucketing") ----
constexpr int kSegCap = 4096;          // touches per cell a workgroup holds (16 per thread)
constexpr int kSegMaxBuckets = 4096;   // LDS histogram of the chunk kernels
constexpr int kSegPosBits = 26, kSegFlShift = 52;
constexpr int64_t kSegMaxCells = (int64_t)1 << 23;
constexpr double kSegMinTouches = 8192.0;  // touches per batch below which bucketing is not tried (tiny batches)
constexpr double kSegTarget = 2048.0;      // touches per cell aimed at (measured +-0 from 500 to 2000: no knob)
constexpr int kSegChunk = 256;             // samples per chunk workgroup: 64 rows per wavefront and trip (seg_walk_rows)
// an item = feature's low bits << sh_fl | position in the batch << sh_pos | entry of the row; 32 bits when the three fit
// (headline: 11 + 13 + 6), else 64 (26 bits each for position and entry)
struct SegFmt {
  int sh_pos, sh_fl;
  uint64_t qmask, pmask;
};

// The column phase walks a batch's unique features in the order of DESCENDING touch count (plan.h); counts of kCntMax and
// more share a class and keep their feature order among themselves.  16 classes: counts differ by a few around their
// mean (Poisson), and a 4-bit class keeps the (batch, class) key of the sort path at two radix passes.
constexpr int kCntClassBits = 4, kCntClasses = 1 << kCntClassBits, kCntMax = kCntClasses - 1;

constexpr int kPlanKnobUnset = INT_MIN;
struct PlanKnobs {  // the table above; every field is kPlanKnobUnset or the variable's atoi()
  int csc = kPlanKnobUnset, key = kPlanKnobUnset, seg = kPlanKnobUnset, seg_fl = kPlanKnobUnset, seg_s = kPlanKnobUnset,
      seg_xcd = kPlanKnobUnset;
};
inline PlanKnobs plan_knobs() {
  const auto knob = [](const char* name) {
    const char* e = getenv(name);
    return e ? atoi(e) : kPlanKnobUnset;
  };
  PlanKnobs k;
  k.csc = knob("NFM_PLAN_CSC");
  k.key = knob("NFM_PLAN_KEY");
  k.seg = knob("NFM_PLAN_SEG");
  k.seg_fl = knob("NFM_SEG_FL");
  k.seg_s = knob("NFM_SEG_S");
  k.seg_xcd = knob("NFM_SEG_XCD");
  return k;
}

// ---- batch bounds ----
// A batch longer than the range is the range: the same boundaries, and what the kernels divide by stays a position
// count -- the column path narrows it to 32 bits (batch_of32), and end - begin + batch overflows near INT64_MAX.
// Plan::batch keeps the caller's value (the plan's key).
inline int64_t plan_eff_batch(int64_t ns, int64_t batch) { return batch > ns && ns >= 0 ? (ns > 1 ? ns : 1) : batch; }

struct PlanBounds {
  int64_t eff = 0;               // what the boundaries and the kernels see: min(batch, max(ns, 1))
  std::vector<int64_t> bat_pos;  // n_batches + 1, relative to begin
  int64_t n_batches = 0, max_batch = 0;
};
// (ns >= 0 and batch >= 1: plan_build checks both first)
inline PlanBounds plan_bounds(int64_t ns, int64_t batch, bool first_singleton) {
  PlanBounds B;
  B.eff = plan_eff_batch(ns, batch);
  B.bat_pos.push_back(0);
  int64_t pos = 0;
  if (first_singleton && ns > 0) { pos = 1; B.bat_pos.push_back(1); }
  while (pos < ns) { pos = pos + B.eff < ns ? pos + B.eff : ns; B.bat_pos.push_back(pos); }
  B.n_batches = (int64_t)B.bat_pos.size() - 1;
  for (int64_t b = 0; b < B.n_batches; ++b)
    if (B.bat_pos[b + 1] - B.bat_pos[b] > B.max_batch) B.max_batch = B.bat_pos[b + 1] - B.bat_pos[b];
  return B;
}

// ---- the (batch, feature) key of the sort ----
// (batch, feature) keys of at most 32 bits -- cfg2: 5 + 17, the headline shape: 11 + 20 -- sort as uint32: a third less
// traffic in every pass of the radix sort and in the passes that read the sorted keys.
// plan_build chooses the key's TYPE before the boundaries exist, from plan_batch_bound(): ceil(ns / eff) + 1 batches, which no
// boundary rule exceeds (the first singleton adds at most one batch), so a key that is narrow by the bound is narrow by the
// count.  The sort's BIT RANGE is taken from the batches there are (Plan::n_batches): never more bits than the type has, and no
// radix pass over bits that are zero in every key.  Plan::key_bits reports the type.
struct PlanKeyBits {
  int fbits, bbits;
  int bits;  // 32 or 64: the key's type when fbits + bbits fit it (more than 64: plan_build refuses, "key overflow")
};
inline int64_t plan_batch_bound(int64_t ns, int64_t eff) { return eff > 0 ? (ns + eff - 1) / eff + 1 : 1; }
inline PlanKeyBits plan_key(int64_t d, int n_aug, int64_t n_batches) {
  PlanKeyBits k{1, 1, 0};
  while (((int64_t)1 << k.fbits) < d + n_aug) ++k.fbits;
  while (((int64_t)1 << k.bbits) < n_batches) ++k.bbits;
  k.bits = k.fbits + k.bbits <= 32 ? 32 : 64;
  return k;
}
// the (batch, count class) key of the per-batch count order: (batch, descending touch count) in 32 bits, the count clamped to
// 4 bits (fewer when there are more than 2^28 batches): two radix passes instead of the five to six of a 64-bit
// (batch << 32 | count) key.  Below 1 the order by count is not made.
inline int plan_count_bits(int bbits) { return bbits <= 32 - kCntClassBits ? kCntClassBits : 32 - bbits; }

// ---- what a build is given ----
struct PlanShape {
  int64_t n, d;        // the dataset
  int max_row;         // its longest row (stored entries)
  int n_aug;
  int64_t begin, end;  // the epoch range
  bool has_order;      // an order was given (host or device)
  bool keyed_order;    // ... and it is gen_permutation's order of a key for exactly this range
  bool use_singles, first_singleton;
  int64_t n_batches, max_batch;  // plan_bounds()
  // the dataset's CscIndex, when the caller has one; built / usable / max_col change when the twin is built
  bool has_csc, csc_built, csc_usable, csc_seg_unfit;
  int64_t csc_max_col;
};
// with an explicit order the range counts positions of the index stream, which may be longer than the data (MBPSGD)
inline bool plan_range_ok(const PlanShape& S) { return S.end - S.begin >= 0 && S.begin >= 0 && (S.end <= S.n || S.has_order); }

// ---- 1. the column-major twin ----
// Dense batches (no singles: every feature a batch touches goes to the column phase), no dummy features, an order
// without repeats: the plan comes from the column-major copy of the data.
struct TwinRoute {
  bool wanted;       // the shape and T ask for the twin
  bool build_first;  // ... which this dataset does not have yet: csc_build runs now (and sets built, usable and max_col)
  bool by_key;       // positions computed from the order's key, not gathered from the table of the inverse order
};
inline TwinRoute twin_route(const PlanShape& S, const PlanKnobs& K, int64_t T) {
  TwinRoute r{};
  r.wanted = K.csc != 0 && S.has_csc && !S.use_singles && S.n_aug == 0 && S.end <= S.n && S.n_batches <= kCscMaxBatches &&
             (double)S.n_batches * (double)S.d <= kCscMaxCells && (double)T >= kCscMinFill * (double)S.n_batches * (double)S.d;
  r.build_first = r.wanted && !S.csc_built;
  r.by_key = K.key != 0 && S.keyed_order;
  return r;
}
// ... and tried when its longest column fits the ranking kernel (S as it is once the twin is built)
inline bool twin_tried(const TwinRoute& r, const PlanShape& S) { return r.wanted && S.csc_usable; }
// entries per lane of k_csc_fill: the launch and Plan::csc_ne
inline int twin_ne(int64_t max_col) { return max_col <= 4 * kPlanWave ? 4 : max_col <= 8 * kPlanWave ? 8 : kCscMaxCol / kPlanWave; }
// k_csc_fill's workgroup for a rung: wavefronts, ints per wavefront, bytes of LDS
struct TwinFill {
  int wpb;
  size_t per_wave, lds_bytes;
};
inline TwinFill twin_fill(int ne, int64_t n_batches) {
  TwinFill f{};
  f.per_wave = (size_t)((4 * ne * kPlanWave + 2 * n_batches + 2) & ~(int64_t)1);
  // at most 48 KB of LDS per workgroup: four wavefronts, or two where four would ask for more -- 16 entries per lane always,
  // and 8 entries per lane at 512 batches (49184 bytes, which used to be launched as it was)
  f.wpb = sizeof(int) * (kPlanBlock / kPlanWave) * f.per_wave > kCscFillLds ? 2 : kPlanBlock / kPlanWave;
  f.lds_bytes = sizeof(int) * f.wpb * f.per_wave;
  return f;
}
// measured by the count pass: the order repeats a sample (an index stream, not a permutation) -- two positions claimed one
// sample, or the touches counted are not the range's T.  The build goes on with bucketing or the sort.
inline bool twin_clashed(unsigned long long clash, int32_t touches, int64_t T) { return clash != 0 || (int64_t)touches != T; }

// ---- 2. bucketing ----
struct SegRoute {
  bool tried;
  int fl;              // bucket width 2^fl
  int64_t nbk, cells;  // buckets, (batch, bucket) cells
  int S, cpb;          // samples per chunk workgroup, chunks per batch
  int pbits, qbits;    // bits of a position in the batch, of an entry of a row
  bool narrow;         // 32-bit items
  SegFmt fmt;
  int xcd;             // one XCD per batch (seg_map)
};
inline SegRoute seg_route(const PlanShape& S, const PlanKnobs& K, int64_t T) {
  SegRoute r{};
  const double bt = (double)T / (double)S.n_batches;  // touches per batch
  if (!(K.seg != 0 && S.n_aug == 0 && bt >= kSegMinTouches && S.max_batch < ((int64_t)1 << kSegPosBits) &&
        S.max_row < (1 << kSegPosBits) && S.d < ((int64_t)1 << 31) && !(S.has_csc && S.csc_seg_unfit)))
    return r;
  int fl = 8;
  while (fl < 12 && (double)(((S.d - 1) >> (fl + 1)) + 1) * kSegTarget >= bt) ++fl;  // the largest bucket count with >= target per cell
  if (K.seg_fl >= 8 && K.seg_fl <= 12) fl = K.seg_fl;
  r.fl = fl;
  r.nbk = ((S.d - 1) >> fl) + 1;
  r.cells = S.n_batches * r.nbk;
  if (!(r.nbk <= kSegMaxBuckets && r.cells <= kSegMaxCells && bt / (double)r.nbk <= 0.75 * kSegCap)) return r;
  r.tried = true;
  r.S = K.seg_s > 0 ? K.seg_s : kSegChunk;
  r.cpb = (int)((S.max_batch + r.S - 1) / r.S);
  int pbits = 1, qbits = 1;
  while (((int64_t)1 << pbits) < S.max_batch) ++pbits;
  while ((1 << qbits) < S.max_row) ++qbits;
  r.pbits = pbits;
  r.qbits = qbits;
  r.narrow = fl + pbits + qbits <= 32;
  r.fmt = r.narrow ? SegFmt{qbits, qbits + pbits, ((uint64_t)1 << qbits) - 1, ((uint64_t)1 << pbits) - 1}
                   : SegFmt{kSegPosBits, kSegFlShift, ((uint64_t)1 << kSegPosBits) - 1, ((uint64_t)1 << kSegPosBits) - 1};
  r.xcd = K.seg_xcd != 0 ? 1 : 0;
  return r;
}
// measured by the count pass: the largest cell.  Beyond what a workgroup holds -- a popular feature -- this dataset's plans
// come from the sort (CscIndex::seg_unfit)
inline bool seg_gives_up(unsigned h_mx) { return h_mx > (unsigned)kSegCap; }
// items per thread of k_seg_classify and k_seg_fill: the launches and Plan::seg_ipt
inline int seg_ipt(unsigned h_mx) { return h_mx <= 4u * kPlanBlock ? 4 : h_mx <= 8u * kPlanBlock ? 8 : kSegCap / kPlanBlock; }
// bytes of LDS of k_seg_fill for a rung
inline size_t seg_fill_lds(int fl, int ipt) {
  const size_t NB = (size_t)1 << fl;
  return sizeof(uint32_t) * (2 * NB + (size_t)kPlanBlock * ipt) + sizeof(uint16_t) * NB;
}

}  // namespace nfm
