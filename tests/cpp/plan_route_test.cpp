// tests/cpp/plan_route_test.cpp -- nimfm_amd/csrc/plan_route.h as a filter: one case per line on stdin, the header's answers per
// line on stdout.  tests/test_cpp_plan_route.py feeds it the cases of tests/plan_route_cases.py and compares with their
// restatement.  Host only: no HIP, no library (g++ -std=c++17; a second build with -fsanitize=address,undefined runs the same
// cases).  With the argument "knobs": what plan_knobs() reads from the environment.  With "parent N SEED": N seeded random draws
// through the header, driven as plan_build drives it, and through parent::plan_build, the decision lines of plan.hip's plan_build
// and plan_build_t as they stood before the header (copied below without the device work: what the device read back is an
// argument; they read the environment themselves, so every draw sets it); prints the number of draws per outcome and every
// disagreement.
//
// in:  B ns batch first_singleton
// out: eff n_batches max_batch bat_pos[1] bat_pos[2] bat_pos[n_batches - 1] sum(bat_pos)          (-1: no such entry)
// in:  K d n_aug ns batch first_singleton
// out: bound fbits bbits bits | n_batches bbits sum cbits       (the key's type by the bound | the sort's bit range by the count)
// in:  R n d max_row n_aug begin end has_order keyed_order use_singles first_singleton n_batches max_batch has_csc csc_built
//        max_col seg_unfit | csc key seg seg_fl seg_s seg_xcd (-2147483648 = unset) | T clash touches (-1: T) h_mx   (without the bars)
// out: range_ok | wanted build_first by_key tried ne wpb per_wave lds_bytes clashed | consulted tried fl nbk cells S cpb pbits qbits
//        narrow sh_pos sh_fl qmask pmask xcd gives_up ipt fill_lds | builder csc_built seg_unfit      (the dataset afterwards)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>

#include "../../nimfm_amd/csrc/plan_route.h"

using namespace nfm;
typedef unsigned long long ull;

// what a build decides, by either side
struct Decided {
  int err = 0;  // 1: the range, 2: the batch, 3: key overflow
  int key_bits = 0, sort_bits = 0, cbits = 0;
  int64_t n_batches = 0, max_batch = 0, bat_sum = 0;
  int csc_built_now = 0, twin_tried = 0, by_key = 0, csc_ne = 0, fill_wpb = 0;
  size_t fill_lds = 0;
  int builder = 0;  // Plan::kBySort = 0, kByTwin = 1, kBySeg = 2
  int seg_tried = 0, seg_fl = 0, seg_item_bits = 0, seg_ipt = 0, seg_s = 0, seg_xcd = 0, cpb = 0;
  int64_t seg_nbk = 0, seg_max_cell = 0;
  SegFmt fmt{};
  int seg_unfit_after = 0;
};

// ---------------------------------------------------------------------------------------------------------------------------
// the parent's lines
// ---------------------------------------------------------------------------------------------------------------------------
namespace parent {
constexpr int kWave = 64, kBlock = 256, kWavesPerBlock = kBlock / kWave;
constexpr int kCntClassBits = 4;
constexpr int kCscMaxCol = 1024;
constexpr int kCscMaxBatches = 512;
constexpr int kSegCap = 4096;
constexpr int kSegMaxBuckets = 4096;
constexpr int kSegPosBits = 26, kSegFlShift = 52;
struct SegFmt {
  int sh_pos, sh_fl;
  uint64_t qmask, pmask;
};
struct CsrView {
  int64_t n, d;
  int32_t max_row;
};
struct CscIndex {
  bool built = false, usable = false;
  bool seg_unfit = false;
  int64_t max_col = 0;
  int64_t true_max_col = 0;  // (what csc_build would find)
};
struct FeistelKey {
  int64_t ns, begin;
};
struct Plan {
  std::vector<int64_t> bat_pos;
  int64_t n_batches = 0, max_batch = 0;
};
static void csc_build(const CsrView&, CscIndex* C) {
  C->max_col = C->true_max_col;
  C->usable = C->max_col <= kCscMaxCol;
  C->built = true;
}

template <class KeyT>
static void plan_build_t(const CsrView& X, int n_aug, const int64_t* perm_host, const int64_t* perm_given_dev, int64_t begin, int64_t end,
                         int64_t batch, bool first_singleton, bool use_singles, CscIndex* csc, const FeistelKey* perm_key,
                         int64_t T, ull h_clash, int32_t T32, unsigned h_mx, Decided& o) {
  Plan P;
  const int64_t ns = end - begin;
  if (!(ns >= 0 && begin >= 0 && (end <= X.n || perm_host || perm_given_dev))) { o.err = 1; return; }
  if (!(batch >= 1)) { o.err = 2; return; }
  o.key_bits = (int)(8 * sizeof(KeyT));
  // batch boundaries
  P.bat_pos.clear();
  P.bat_pos.push_back(0);
  int64_t pos = 0;
  if (first_singleton && ns > 0) { pos = 1; P.bat_pos.push_back(1); }
  while (pos < ns) { pos = pos + batch < ns ? pos + batch : ns; P.bat_pos.push_back(pos); }
  P.n_batches = (int64_t)P.bat_pos.size() - 1;
  P.max_batch = 0;
  for (int64_t b = 0; b < P.n_batches; ++b) P.max_batch = std::max(P.max_batch, P.bat_pos[b + 1] - P.bat_pos[b]);
  o.n_batches = P.n_batches, o.max_batch = P.max_batch;
  for (int64_t v : P.bat_pos) o.bat_sum += v;
  if (ns == 0) return;
  if (T == 0) return;
  int fbits = 1;
  while (((int64_t)1 << fbits) < X.d + n_aug) ++fbits;
  int bbits = 1;
  while (((int64_t)1 << bbits) < P.n_batches) ++bbits;
  if (!(fbits + bbits <= 64)) { o.err = 3; return; }
  o.sort_bits = fbits + bbits;
  const bool csc_on = !(getenv("NFM_PLAN_CSC") && atoi(getenv("NFM_PLAN_CSC")) == 0);
  bool use_csc = csc_on && csc && !use_singles && n_aug == 0 && end <= X.n && P.n_batches <= kCscMaxBatches &&
                 (double)P.n_batches * (double)X.d <= 268435456.0 && (double)T >= 0.5 * (double)P.n_batches * (double)X.d;
  if (use_csc && !csc->built) { csc_build(X, csc); o.csc_built_now = 1; }
  use_csc = use_csc && csc->usable;
  if (use_csc) {
    o.twin_tried = 1;
    const bool key_on = !(getenv("NFM_PLAN_KEY") && atoi(getenv("NFM_PLAN_KEY")) == 0);  // 0: the table, also for device-drawn orders
    const bool by_key = key_on && perm_key != nullptr && perm_key->ns == ns && perm_key->begin == begin;
    if (h_clash != 0 || (int64_t)T32 != T) {
      use_csc = false;  // the order repeats a sample (an index stream, not a permutation): the general path below
    } else {
      auto fill = [&](auto ne_tag) {
        constexpr int NE = decltype(ne_tag)::value;
        const size_t per_wave = (size_t)((4 * NE * kWave + 2 * P.n_batches + 2) & ~(int64_t)1);
        const int wpb = NE > 8 ? 2 : kWavesPerBlock;  // at most 48 KB of LDS per workgroup
        o.fill_wpb = wpb;
        o.fill_lds = sizeof(int) * wpb * per_wave;
      };
      if (csc->max_col <= 4 * kWave) fill(std::integral_constant<int, 4>{});
      else if (csc->max_col <= 8 * kWave) fill(std::integral_constant<int, 8>{});
      else fill(std::integral_constant<int, kCscMaxCol / kWave>{});
      o.builder = 1;
      o.csc_ne = csc->max_col <= 4 * kWave ? 4 : csc->max_col <= 8 * kWave ? 8 : kCscMaxCol / kWave;
      o.by_key = by_key;
    }
  }
  bool use_seg = false;
  {
    const char* e = getenv("NFM_PLAN_SEG");  // read per build: the tests switch it
    const bool seg_on = !(e && atoi(e) == 0);
    const double bt = (double)T / (double)P.n_batches;  // touches per batch
    if (!use_csc && seg_on && n_aug == 0 && bt >= 8192.0 && P.max_batch < ((int64_t)1 << kSegPosBits) &&
        X.max_row < (1 << kSegPosBits) && X.d < ((int64_t)1 << 31) && !(csc && csc->seg_unfit)) {
      const int fl_env = getenv("NFM_SEG_FL") ? atoi(getenv("NFM_SEG_FL")) : 0;
      const double target = 2048.0;  // touches per cell aimed at (measured +-0 from 500 to 2000: no knob)
      int fl = 8;
      while (fl < 12 && (double)(((X.d - 1) >> (fl + 1)) + 1) * target >= bt) ++fl;  // the largest bucket count with >= target per cell
      if (fl_env >= 8 && fl_env <= 12) fl = fl_env;
      const int64_t nbk = ((X.d - 1) >> fl) + 1;
      const int64_t cells = P.n_batches * nbk;
      if (nbk <= kSegMaxBuckets && cells <= ((int64_t)1 << 23) && bt / (double)nbk <= 0.75 * kSegCap) {
        o.seg_tried = 1;
        const int s_env = getenv("NFM_SEG_S") ? atoi(getenv("NFM_SEG_S")) : 0;
        const int S = s_env > 0 ? s_env : 256;  // samples per chunk workgroup: 64 rows per wavefront and trip (seg_walk_rows)
        o.cpb = (int)((P.max_batch + S - 1) / S);
        int pbits = 1, qbits = 1;
        while (((int64_t)1 << pbits) < P.max_batch) ++pbits;
        while ((1 << qbits) < X.max_row) ++qbits;
        const bool narrow = fl + pbits + qbits <= 32;
        const SegFmt fmt = narrow ? SegFmt{qbits, qbits + pbits, ((uint64_t)1 << qbits) - 1, ((uint64_t)1 << pbits) - 1}
                                  : SegFmt{kSegPosBits, kSegFlShift, ((uint64_t)1 << kSegPosBits) - 1, ((uint64_t)1 << kSegPosBits) - 1};
        o.fmt = ::SegFmt{fmt.sh_pos, fmt.sh_fl, fmt.qmask, fmt.pmask};
        const int xcd = !(getenv("NFM_SEG_XCD") && atoi(getenv("NFM_SEG_XCD")) == 0) ? 1 : 0;
        o.seg_fl = fl;
        o.seg_nbk = (int)nbk;
        o.seg_max_cell = (int64_t)h_mx;
        if (h_mx > (unsigned)kSegCap) {
          if (csc) csc->seg_unfit = true;  // a popular feature: this dataset's plans come from the sort
        } else {
          use_seg = true;
          o.builder = 2;
          o.seg_item_bits = narrow ? 32 : 64;
          o.seg_ipt = h_mx <= 4 * kBlock ? 4 : h_mx <= 8 * kBlock ? 8 : kSegCap / kBlock;
          o.seg_s = S;
          o.seg_xcd = xcd;
        }
      }
    }
  }
  (void)use_seg;
  o.cbits = bbits <= 32 - kCntClassBits ? kCntClassBits : 32 - bbits;
  o.seg_unfit_after = csc && csc->seg_unfit;
}

static void plan_build(const CsrView& X, int n_aug, const int64_t* perm_host, int64_t begin, int64_t end, int64_t batch, bool first_singleton,
                       bool use_singles, const int64_t* perm_dev, CscIndex* csc, const FeistelKey* perm_key, int64_t T, ull h_clash, int32_t T32,
                       unsigned h_mx, Decided& o) {
  int fbits = 1, bbits = 1;
  while (((int64_t)1 << fbits) < X.d + n_aug) ++fbits;
  const int64_t ns = end - begin;
  const int64_t eff = batch > ns && ns >= 0 ? std::max<int64_t>(ns, 1) : batch;
  const int64_t nb = eff > 0 ? (ns + eff - 1) / eff + 1 : 1;
  while (((int64_t)1 << bbits) < nb) ++bbits;
  if (fbits + bbits <= 32)
    return plan_build_t<uint32_t>(X, n_aug, perm_host, perm_dev, begin, end, eff, first_singleton, use_singles, csc, perm_key, T, h_clash, T32, h_mx, o);
  return plan_build_t<uint64_t>(X, n_aug, perm_host, perm_dev, begin, end, eff, first_singleton, use_singles, csc, perm_key, T, h_clash, T32, h_mx, o);
}
}  // namespace parent

// ---------------------------------------------------------------------------------------------------------------------------
// the header, driven as plan.hip's plan_build and plan_prologue drive it
// ---------------------------------------------------------------------------------------------------------------------------
struct Csc {
  bool built, usable, seg_unfit;
  int64_t max_col, true_max_col;
};
static void see_csc(PlanShape& S, const Csc* csc) {
  S.has_csc = csc != nullptr;
  if (csc) S.csc_built = csc->built, S.csc_usable = csc->usable, S.csc_max_col = csc->max_col, S.csc_seg_unfit = csc->seg_unfit;
}
// S: everything but n_batches and max_batch
static void drive(PlanShape S, int64_t batch, Csc* csc, int64_t T, ull h_clash, int32_t T32, unsigned h_mx, Decided& o) {
  const int64_t ns = S.end - S.begin;
  const int64_t eff = plan_eff_batch(ns, batch);
  see_csc(S, csc);
  if (!plan_range_ok(S)) { o.err = 1; return; }
  if (!(eff >= 1)) { o.err = 2; return; }
  o.key_bits = plan_key(S.d, S.n_aug, plan_batch_bound(ns, eff)).bits;
  const PlanBounds B = plan_bounds(ns, batch, S.first_singleton);
  S.n_batches = o.n_batches = B.n_batches, S.max_batch = o.max_batch = B.max_batch;
  for (int64_t v : B.bat_pos) o.bat_sum += v;
  if (ns == 0 || T == 0) return;
  const PlanKeyBits key = plan_key(S.d, S.n_aug, B.n_batches);
  if (!(key.fbits + key.bbits <= 64)) { o.err = 3; return; }
  o.sort_bits = key.fbits + key.bbits;
  const PlanKnobs K = plan_knobs();
  bool built = false;
  const TwinRoute tw = twin_route(S, K, T);
  if (tw.build_first) {
    csc->max_col = csc->true_max_col, csc->usable = csc->max_col <= kCscMaxCol, csc->built = true;
    o.csc_built_now = 1;
    see_csc(S, csc);
  }
  if (twin_tried(tw, S)) {
    o.twin_tried = 1;
    if (!twin_clashed(h_clash, T32, T)) {
      built = true;
      o.builder = 1, o.csc_ne = twin_ne(csc->max_col), o.by_key = tw.by_key;
      const TwinFill f = twin_fill(o.csc_ne, B.n_batches);
      o.fill_wpb = f.wpb, o.fill_lds = f.lds_bytes;
    }
  }
  if (!built) {
    const SegRoute sg = seg_route(S, K, T);
    if (sg.tried) {
      o.seg_tried = 1, o.cpb = sg.cpb, o.fmt = sg.fmt, o.seg_fl = sg.fl, o.seg_nbk = sg.nbk, o.seg_max_cell = h_mx;
      if (seg_gives_up(h_mx)) {
        if (csc) csc->seg_unfit = true;
      } else {
        built = true;
        o.builder = 2, o.seg_item_bits = sg.narrow ? 32 : 64, o.seg_ipt = seg_ipt(h_mx), o.seg_s = sg.S, o.seg_xcd = sg.xcd;
      }
    }
  }
  o.cbits = plan_count_bits(key.bbits);
  o.seg_unfit_after = csc && csc->seg_unfit;
}

static void put_env(const char* name, int v) {
  if (v == kPlanKnobUnset) unsetenv(name);
  else setenv(name, std::to_string(v).c_str(), 1);
}

static long long n_bad = 0;
#define SAME(what, a, b)                                                                              \
  do {                                                                                                \
    if ((long long)(a) != (long long)(b) && n_bad++ < 40)                                             \
      printf("DISAGREE draw %d %s: header %lld parent %lld\n", draw, what, (long long)(a), (long long)(b)); \
  } while (0)

static int parent_draws(int n, unsigned seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&](std::initializer_list<long long> v) { return *(v.begin() + rng() % v.size()); };
  long long seen_corner = 0;  // draws at the one rung and batch count where the parent's k_csc_fill asked for more than 48 KB
  long long seen[10] = {0};  // twin, twin tried and clashed, seg, seg gave up, sort, key 64, errors, narrow, wide, csc built now
  const int64_t P26 = (int64_t)1 << 26, P31 = (int64_t)1 << 31;
  for (int draw = 0; draw < n; ++draw) {
    PlanShape S{};
    S.d = pick({1, 2, 8, 37, 4096, 8192 - 37, 16384 - 5, 65536, 1 << 19, (1 << 19) + 1, 1 << 20, 1 << 24, (1 << 24) + 1, 1 << 28, P31 - 1, P31, P31 + 1});
    S.max_row = (int)pick({1, 6, 24, 63, 64, 65, 200, (1 << 13) - 1, 1 << 13, P26 - 1, P26});
    S.n_aug = (int)pick({0, 0, 0, 0, 1, 2});
    S.first_singleton = rng() % 4 == 0;
    S.use_singles = rng() % 3 == 0;
    const bool dense = rng() % 16 == 0;  // a family the twin takes: few features in every row, batches of two around 512 of them
    if (dense) S.d = 8, S.n_aug = 0, S.first_singleton = false, S.use_singles = false;
    // the batch, then a range of at most 70000 batches around the thresholds of the batch count
    int64_t batch = pick({0, -3, 1, 2, 16, 500, 8192, 8193, 16384, 16385, P26 - 1, P26, P26 + 1, (int64_t)1 << 32, ((int64_t)1 << 32) + 7, INT64_MAX});
    int64_t nb_aim = pick({0, 1, 2, 3, 64, 511, 512, 513, 1000, 2048, 2049, 4095, 4096, 32768, 32769, 65536});
    if (dense) batch = 2, nb_aim = pick({496, 511, 512, 512, 513});
    int64_t ns = batch >= 1 && batch <= P26 + 1 ? std::min<int64_t>(nb_aim * batch + (int64_t)pick({0, 0, 1, -1}), (int64_t)1 << 40) : nb_aim;
    if (rng() % 40 == 0) ns = -1;
    S.begin = pick({0, 0, 0, 17, 100});
    if (rng() % 60 == 0) S.begin = -1;
    S.end = S.begin + ns;
    S.n = rng() % 6 == 0 ? S.end - (int64_t)pick({1, 5}) : S.end + (int64_t)pick({0, 0, 3});
    const int order = (int)pick({0, 1, 1, 2});  // none, host, device
    S.has_order = order != 0;
    const parent::FeistelKey fk{rng() % 8 == 0 ? ns + 1 : ns, rng() % 8 == 0 ? S.begin + 1 : S.begin};
    const bool give_key = order == 2 && rng() % 8 != 0;
    S.keyed_order = give_key && fk.ns == ns && fk.begin == S.begin;
    const bool have_csc = dense || rng() % 6 != 0;
    Csc c1{rng() % 2 == 0, false, rng() % 8 == 0, 0, (int64_t)pick({0, 1, 255, 256, 257, 512, 513, 1023, 1024, 1025, 4000})};
    if (c1.built) c1.max_col = c1.true_max_col, c1.usable = c1.max_col <= kCscMaxCol;
    parent::CscIndex c2;
    c2.built = c1.built, c2.usable = c1.usable, c2.seg_unfit = c1.seg_unfit, c2.max_col = c1.max_col, c2.true_max_col = c1.true_max_col;
    PlanKnobs K;
    K.csc = (int)pick({kPlanKnobUnset, kPlanKnobUnset, kPlanKnobUnset, 0, 1});
    K.key = (int)pick({kPlanKnobUnset, kPlanKnobUnset, 0, 1});
    K.seg = (int)pick({kPlanKnobUnset, kPlanKnobUnset, kPlanKnobUnset, 0, 1});
    K.seg_fl = (int)pick({kPlanKnobUnset, kPlanKnobUnset, kPlanKnobUnset, 0, 7, 8, 9, 10, 11, 12, 13});
    K.seg_s = (int)pick({kPlanKnobUnset, kPlanKnobUnset, 0, -1, 1, 64, 256, 1000});
    K.seg_xcd = (int)pick({kPlanKnobUnset, kPlanKnobUnset, 0, 1, 2});
    put_env("NFM_PLAN_CSC", K.csc), put_env("NFM_PLAN_KEY", K.key), put_env("NFM_PLAN_SEG", K.seg);
    put_env("NFM_SEG_FL", K.seg_fl), put_env("NFM_SEG_S", K.seg_s), put_env("NFM_SEG_XCD", K.seg_xcd);
    {
      const PlanKnobs e = plan_knobs();
      SAME("knobs", e.csc == K.csc && e.key == K.key && e.seg == K.seg && e.seg_fl == K.seg_fl && e.seg_s == K.seg_s && e.seg_xcd == K.seg_xcd, 1);
    }
    // T around the thresholds the batch count and d set: half of the (batch, feature) cells, 8192 per batch, the fl ladder,
    // 3072 per cell
    const int64_t eff = plan_eff_batch(ns, batch);
    const int64_t nb = ns > 0 && eff >= 1 ? (ns + eff - 1) / eff + (S.first_singleton ? 1 : 0) : 1;
    const int fl_pick = (int)pick({8, 9, 10, 11, 12});
    const int64_t nbk = ((S.d - 1) >> fl_pick) + 1;
    const double aims[] = {0.5 * (double)nb * (double)S.d, 8192.0 * (double)nb, (double)((((S.d - 1) >> (fl_pick + 1)) + 1) * 2048) * (double)nb,
                           3072.0 * (double)nbk * (double)nb, 60000.0};
    double Td = aims[dense ? 0 : rng() % 5] + (double)pick({0, 0, -1, 1, -(long long)nb, (long long)nb, 1000});
    if (rng() % 30 == 0) Td = 0;
    const int64_t T = (int64_t)std::min(std::max(Td, 0.0), 2147483646.0);
    const ull h_clash = rng() % 8 == 0 ? 1 + rng() % 3 : 0;
    const int32_t T32 = rng() % 10 == 0 ? (int32_t)(T + (int64_t)pick({-1, 1, 7})) : (int32_t)T;
    const unsigned h_mx = (unsigned)pick({0, 1, 600, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 100000});
    Decided a, b;
    drive(S, batch, have_csc ? &c1 : nullptr, T, h_clash, T32, h_mx, a);
    const parent::CsrView X{S.n, S.d, S.max_row};
    const int64_t dummy = 0;
    parent::plan_build(X, S.n_aug, order == 1 ? &dummy - S.begin : nullptr, S.begin, S.end, batch, S.first_singleton, S.use_singles,
                       order == 2 ? &dummy : nullptr, have_csc ? &c2 : nullptr, give_key ? &fk : nullptr, T, h_clash, T32, h_mx, b);
    SAME("err", a.err, b.err); SAME("key_bits", a.key_bits, b.key_bits); SAME("sort_bits", a.sort_bits, b.sort_bits); SAME("cbits", a.cbits, b.cbits);
    SAME("n_batches", a.n_batches, b.n_batches); SAME("max_batch", a.max_batch, b.max_batch); SAME("bat_sum", a.bat_sum, b.bat_sum);
    SAME("csc_built_now", a.csc_built_now, b.csc_built_now); SAME("twin_tried", a.twin_tried, b.twin_tried); SAME("by_key", a.by_key, b.by_key);
    SAME("csc_ne", a.csc_ne, b.csc_ne);
    // k_csc_fill's workgroup is the parent's wherever the parent kept to the 48 KB its comment names; the one place it did not
    // (8 entries per lane, 512 batches: 49184 bytes in four wavefronts) is two wavefronts now, half the bytes
    if (b.fill_lds <= 48 * 1024) {
      SAME("fill_wpb", a.fill_wpb, b.fill_wpb); SAME("fill_lds", a.fill_lds, b.fill_lds);
    } else {
      SAME("fill corner", b.csc_ne == 8 && b.n_batches == 512 && b.fill_lds == 49184, 1);
      SAME("fill_wpb halved", a.fill_wpb, 2); SAME("fill_lds halved", 2 * a.fill_lds, b.fill_lds);
      ++seen_corner;
    }
    SAME("builder", a.builder, b.builder); SAME("seg_tried", a.seg_tried, b.seg_tried); SAME("seg_fl", a.seg_fl, b.seg_fl);
    SAME("seg_nbk", a.seg_nbk, b.seg_nbk); SAME("seg_max_cell", a.seg_max_cell, b.seg_max_cell); SAME("seg_item_bits", a.seg_item_bits, b.seg_item_bits);
    SAME("seg_ipt", a.seg_ipt, b.seg_ipt); SAME("seg_s", a.seg_s, b.seg_s); SAME("seg_xcd", a.seg_xcd, b.seg_xcd); SAME("cpb", a.cpb, b.cpb);
    SAME("sh_pos", a.fmt.sh_pos, b.fmt.sh_pos); SAME("sh_fl", a.fmt.sh_fl, b.fmt.sh_fl); SAME("qmask", a.fmt.qmask, b.fmt.qmask);
    SAME("pmask", a.fmt.pmask, b.fmt.pmask); SAME("seg_unfit_after", a.seg_unfit_after, b.seg_unfit_after);
    SAME("csc built", c1.built, c2.built); SAME("csc usable", c1.usable, c2.usable); SAME("csc max_col", c1.max_col, c2.max_col);
    SAME("csc seg_unfit", c1.seg_unfit, c2.seg_unfit);
    seen[0] += b.builder == 1, seen[1] += b.twin_tried && b.builder != 1, seen[2] += b.builder == 2, seen[3] += b.seg_tried && b.builder != 2;
    seen[4] += !b.err && b.sort_bits && b.builder == 0, seen[5] += b.key_bits == 64, seen[6] += b.err != 0;
    seen[7] += b.seg_item_bits == 32, seen[8] += b.seg_item_bits == 64, seen[9] += b.csc_built_now;
  }
  printf("draws %d disagreements %lld | twin %lld clashed %lld seg %lld gave_up %lld sort %lld | key64 %lld errors %lld narrow %lld wide %lld built_now %lld fill_corner %lld\n",
         n, n_bad, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5], seen[6], seen[7], seen[8], seen[9], seen_corner);
  return n_bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "knobs") == 0) {
    const PlanKnobs k = plan_knobs();
    printf("%d %d %d %d %d %d\n", k.csc, k.key, k.seg, k.seg_fl, k.seg_s, k.seg_xcd);
    return 0;
  }
  if (argc > 3 && strcmp(argv[1], "parent") == 0) return parent_draws(atoi(argv[2]), (unsigned)atoi(argv[3]));
  long long n_lines = 0;
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'B') {
      long long ns, batch;
      int fs;
      if (scanf("%lld %lld %d", &ns, &batch, &fs) != 3) return 2;
      const PlanBounds B = plan_bounds(ns, batch, fs != 0);
      long long sum = 0;
      for (int64_t v : B.bat_pos) sum += v;
      const auto at = [&](int64_t i) { return i >= 1 && i <= B.n_batches ? (long long)B.bat_pos[i] : -1ll; };
      printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)B.eff, (long long)B.n_batches, (long long)B.max_batch, at(1), at(2), at(B.n_batches - 1), sum);
    } else if (kind[0] == 'K') {
      long long d, ns, batch;
      int n_aug, fs;
      if (scanf("%lld %d %lld %lld %d", &d, &n_aug, &ns, &batch, &fs) != 5) return 2;
      const int64_t bound = plan_batch_bound(ns, plan_eff_batch(ns, batch));
      const PlanKeyBits t = plan_key(d, n_aug, bound);
      const int64_t nb = plan_bounds(ns, batch, fs != 0).n_batches;
      const PlanKeyBits s = plan_key(d, n_aug, nb);
      printf("%lld %d %d %d | %lld %d %d %d\n", (long long)bound, t.fbits, t.bbits, t.bits, (long long)nb, s.bbits, s.fbits + s.bbits, plan_count_bits(s.bbits));
    } else if (kind[0] == 'R') {
      PlanShape S{};
      PlanKnobs K;
      long long n, d, begin, end, nb, mb, max_col, T, touches;
      unsigned long long clash, h_mx;
      int has_order, keyed, singles, fs, has_csc, built, unfit;
      const int got = scanf("%lld %lld %d %d %lld %lld %d %d %d %d %lld %lld %d %d %lld %d %d %d %d %d %d %d %lld %llu %lld %llu", &n, &d, &S.max_row, &S.n_aug,
                            &begin, &end, &has_order, &keyed, &singles, &fs, &nb, &mb, &has_csc, &built, &max_col, &unfit, &K.csc, &K.key, &K.seg,
                            &K.seg_fl, &K.seg_s, &K.seg_xcd, &T, &clash, &touches, &h_mx);
      if (got != 26) {
        fprintf(stderr, "line %lld: %d of 26 fields\n", n_lines + 1, got);
        return 2;
      }
      S.n = n, S.d = d, S.begin = begin, S.end = end, S.has_order = has_order, S.keyed_order = keyed, S.use_singles = singles, S.first_singleton = fs;
      S.n_batches = nb, S.max_batch = mb;
      Csc csc{built != 0, built != 0 && max_col <= kCscMaxCol, unfit != 0, built ? max_col : 0, max_col};
      see_csc(S, has_csc ? &csc : nullptr);
      const TwinRoute tw = twin_route(S, K, T);
      if (tw.build_first) {
        csc.built = true, csc.max_col = csc.true_max_col, csc.usable = csc.max_col <= kCscMaxCol;
        see_csc(S, &csc);
      }
      const bool tried = twin_tried(tw, S);
      const int ne = twin_ne(max_col);
      const TwinFill f = twin_fill(ne, nb);
      const bool clashed = tried && twin_clashed(clash, (int32_t)(touches < 0 ? T : touches), T);
      int builder = tried && !clashed ? 1 : 0;
      printf("%d | %d %d %d %d %d %d %zu %zu %d | ", (int)plan_range_ok(S), (int)tw.wanted, (int)tw.build_first, (int)tw.by_key, (int)tried, ne, f.wpb, f.per_wave,
             f.lds_bytes, (int)clashed);
      SegRoute sg{};
      const bool consulted = builder == 0;
      if (consulted) sg = seg_route(S, K, T);
      const bool gives_up = seg_gives_up((unsigned)h_mx);
      const int ipt = seg_ipt((unsigned)h_mx);
      if (sg.tried && gives_up && has_csc) csc.seg_unfit = true;
      if (sg.tried && !gives_up) builder = 2;
      printf("%d %d %d %lld %lld %d %d %d %d %d %d %d %llu %llu %d %d %d %zu | ", (int)consulted, (int)sg.tried, sg.fl, (long long)sg.nbk, (long long)sg.cells, sg.S,
             sg.cpb, sg.pbits, sg.qbits, (int)sg.narrow, sg.fmt.sh_pos, sg.fmt.sh_fl, (ull)sg.fmt.qmask, (ull)sg.fmt.pmask, sg.xcd, (int)gives_up, ipt,
             seg_fill_lds(sg.fl ? sg.fl : 8, ipt));
      printf("%d %d %d\n", builder, (int)csc.built, (int)csc.seg_unfit);
    } else {
      return 2;
    }
    ++n_lines;
  }
  fprintf(stderr, "plan_route: %lld cases\n", n_lines);
  return 0;
}
