// tests/cpp/seq_route_test.cpp -- nimfm_amd/csrc/seq_route.h as a filter: one case per line on stdin; the window's route and the
// one-workgroup route per line on stdout.  tests/test_cpp_seq_route.py feeds it the cases of tests/seq_route_cases.py and compares
// with their restatement.  Host only: no HIP, no library (g++ -std=c++17; a second build with -fsanitize=address,undefined runs
// the same cases).  With the argument "knobs": what seq_knobs() reads from the environment.  With "parent N SEED": N seeded random
// draws through the header and through parent_*, the decision lines of seqwin.hip, api.hip and seq.hip as they stood before the
// header (copied below with ModelView cut down to what they read; they read the environment themselves, so every draw sets it);
// prints the number of draws per outcome and every disagreement.
//
// in:  kind degree nb kc k Kp n_aug fit_intercept d da bs rs m_cap ns nnz ada n_cu | win exact nocond w par trace pipe stage
//      (-2147483648 = unset) | fallbacks snap_bytes   (without the bars)
// out: two_block nb Kp supported reason offered no_cond one_term wk W lgW first_worker m_cap lgKp terms ch FW np thr near_r par_min
//      lds_worker lds_cond lds_bytes n_fwd n_res n_ctl n_partial n_fw n_fw_tags n_scales fits_cus fits counter |
//      refusal step m_cap T threads S lgS rc split_terms lds_bytes table_in_lds table_bytes counter   ("-": no counter)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "../../nimfm_amd/csrc/seq_route.h"

using namespace nfm;

// ---------------------------------------------------------------------------------------------------------------------------
// the parent's lines
// ---------------------------------------------------------------------------------------------------------------------------
namespace parent {
constexpr int kWave = 64;
enum { NFM_KIND_FM = 0, NFM_KIND_FFM = 1 };
namespace dev { constexpr int kMaxDeg = 6; }
typedef unsigned long long ull;
constexpr int kWinRing = 8, kWinDepth = 8, kWinHdr = 4, kWinMaxNL = 5, kSumGran = 13, kSumRing = 256, kResWords = 4;
constexpr int kFwVals = 3;
constexpr size_t kFwRows = (size_t)kWave * 4;
constexpr size_t kFwLin = kFwRows + (size_t)kFwVals * kWave * kWave * 2;
constexpr size_t kFwSlot = kFwLin + (size_t)5 * kWave * 2;
enum { WK_GENERAL = 0, WK_K64 = 1, WK_FFM = 2, WK_FMX = 3 };
constexpr int kSeqMaxDeg = 8, kPipeThreads = 256, kPipeThreadsWide = 512, kPipePairCap = 4096;

struct ModelView {
  int64_t d, da;
  int32_t nb, k, Kp, L, degree, n_aug, kind, fit_intercept, kc;
  int64_t bs, rs;
};

static int win_ffm_terms(int m_cap) { return m_cap + m_cap * (m_cap - 1) / 2; }
static size_t win_worker_lds(int wk, const ModelView& M, int m_cap, bool ada, int W) {
  const WinShape s{M.Kp, win_lg(M.Kp), M.nb, M.k, m_cap, ada, W};
  return wk == WK_K64 ? win_k64_lds(s).total : wk == WK_GENERAL ? win_general_lds(s).total : win_slots_lds(s, wk == WK_FFM).total;
}
static bool win_no_cond(const ModelView& M) {
  const char* env = getenv("NFM_SEQ_WIN_NOCOND");
  return !(env && atoi(env) == 0) && !M.fit_intercept;
}
static bool win_one_term(const ModelView& M) {
  const char* env = getenv("NFM_SEQ_WIN_EXACT");
  return !win_no_cond(M) && !(env && atoi(env) != 0);
}
static ModelView seq_window_view(const ModelView& M) {
  const char* exact = getenv("NFM_SEQ_WIN_EXACT");
  if (exact && atoi(exact) != 0) return M;
  if (!(M.kind == NFM_KIND_FM && M.degree == 2 && M.n_aug == 0 && M.Kp == 2 * kWave)) return M;
  const bool one_block = M.nb == 1 && M.kc == 1 && M.bs == M.da && M.rs == 1;
  const bool wide_rows = M.kc > 1 && M.nb == M.kc && M.bs == 1 && M.rs == M.nb;
  if (!one_block && !wide_rows) return M;
  ModelView V = M;
  V.nb = 2 * M.nb;
  V.kc = V.nb;
  V.Kp = kWave;
  V.L = kWave / 2;
  V.k = kWave;
  V.bs = 1;
  V.rs = V.nb;
  return V;
}
static bool seq_window_supported(const ModelView& M, int m_cap, int64_t ns, int64_t nnz, int n_cu, bool ada) {
  const char* env = getenv("NFM_SEQ_WIN");
  const int mode = env ? atoi(env) : 1;
  if (mode == 0) return false;
  if (M.Kp > kWave || M.Kp < 2) return false;
  const bool term_mail = !(win_no_cond(M) || win_one_term(M));
  if (M.kind == NFM_KIND_FFM) {
    if (M.n_aug != 0 || M.nb < 1 || m_cap < 1) return false;
    if (term_mail && kWinHdr + (win_ffm_terms(m_cap) + 63) / 64 * 64 > kWave * kWinMaxNL) return false;
    if (win_worker_lds(WK_FFM, M, m_cap, ada, kWinLdsSupportWSlots) > 160 * 1024) return false;
  } else if (M.kind == NFM_KIND_FM && (M.nb != 1 || M.degree != 2)) {
    if (M.n_aug != 0 || M.nb < 1 || M.degree < 2 || M.degree > dev::kMaxDeg || m_cap < 1) return false;
    if (term_mail && kWinHdr + (m_cap + M.nb + 63) / 64 * 64 > kWave * kWinMaxNL) return false;
    if (win_worker_lds(WK_FMX, M, m_cap, ada, kWinLdsSupportWSlots) > 160 * 1024) return false;
  } else {
    if (M.kind != NFM_KIND_FM || M.nb != 1 || M.degree != 2 || M.n_aug != 0) return false;
    if (term_mail && kWinHdr + (m_cap + 63) / 64 * 64 > kWave * kWinMaxNL) return false;
    if (!(M.Kp == kWave && m_cap <= kWave) && win_worker_lds(WK_GENERAL, M, m_cap, ada, kWinLdsSupportW) > 160 * 1024) return false;
  }
  if (nnz >= ((int64_t)1 << 32) || M.d >= ((int64_t)1 << 31) || ns >= ((int64_t)1 << 31)) return false;
  if (n_cu < 17) return false;
  return mode == 2 || ns >= 2048;
}
// api.hip: seq_window_offered up to the allocation (have_seqwin: the optimizer has launched a window before)
static bool seq_window_offered(const ModelView& Mw, int m_cap, int64_t ns, int64_t nnz, int n_cu, bool ada, bool have_seqwin, int64_t fallbacks,
                               size_t snap_bytes) {
  const char* win_env = getenv("NFM_SEQ_WIN");
  const bool snap_pays = (win_env && atoi(win_env) == 2) || (double)ns * 0.8e-6 * 0.25 >= (double)snap_bytes / 2.0e12;
  const bool win_trusted = !have_seqwin || fallbacks < 2;
  if (!(snap_pays && win_trusted && seq_window_supported(Mw, m_cap, ns, nnz, n_cu, ada))) return false;
  return true;
}
struct Launch {  // what launch_sequential_window worked out before its loop; fallback: 1 = at the CU check, 2 = at the LDS check
  int fallback, W, lgW, no_cond, first_worker, one_term, par_min, np, thr, near_r, m_cap, FW, lgKp, ch, wk, terms, trace;
  size_t n_fwd, n_res, mail_bytes, ctl_bytes, ctl_zeroed, scales_bytes, fw_bytes, fw_zeroed, lds_worker, lds_cond, lds_bytes;
};
static Launch launch_sequential_window(int n_cu, bool ada, const ModelView& M, int64_t ns, int m_cap, int64_t sw_fallbacks) {
  Launch a{};
  if (m_cap < 1) m_cap = 1;
  const bool no_cond = win_no_cond(M);
  bool one_term = win_one_term(M);
  const bool k64_shape = M.kind == NFM_KIND_FM && M.nb == 1 && M.degree == 2 && M.Kp == kWave && m_cap <= kWave;
  int W = no_cond || k64_shape ? 128 : 64;
  if (no_cond && M.kind == NFM_KIND_FM && M.nb == 1 && M.degree == 2 && M.Kp == kWave && m_cap <= kWave && sw_fallbacks == 0) W = 256;
  if (const char* env = getenv("NFM_SEQ_WIN_W")) W = atoi(env);
  int lgW = 4;
  while ((2 << lgW) <= W && lgW < (no_cond ? 8 : 7)) ++lgW;
  W = 1 << lgW;
  const int extra = no_cond ? 0 : 1;
  while (W + extra > n_cu && lgW > 4) W = 1 << --lgW;
  if (!(W > kWinDepth && W + extra <= n_cu)) return a.fallback = 1, a;
  const int lgKp = win_lg(M.Kp);
  const bool ffm = M.kind == NFM_KIND_FFM;
  const bool fmx = !ffm && (M.nb != 1 || M.degree != 2);
  const int terms = ffm ? win_ffm_terms(m_cap) : fmx ? m_cap + M.nb : m_cap;
  const int ch = one_term || terms <= 32 ? 32 : 64;
  const int FW = one_term ? kWinHdr + 32 : kWinHdr + (terms + ch - 1) / ch * ch;
  const bool k64 = !ffm && !fmx && M.Kp == kWave && m_cap <= kWave;
  const int wk = ffm ? WK_FFM : fmx ? WK_FMX : k64 ? WK_K64 : WK_GENERAL;
  const int np = no_cond ? 4 : 2;
  const size_t n_fwd = one_term ? (size_t)kSumGran * np * W : (size_t)W * np * FW, n_res = (size_t)W * np * kResWords;
  a.mail_bytes = sizeof(ull) * (n_fwd + n_res);
  a.ctl_bytes = sizeof(unsigned) * (W + 64) + sizeof(double) * 2 * (W + 1) + sizeof(int64_t) * 2;
  if (!ada) a.scales_bytes = sizeof(double) * 2 * (size_t)ns;
  a.fw_bytes = sizeof(ull) * (kFwSlot * np + 2 * kWave) * (size_t)W;
  a.trace = getenv("NFM_SEQ_WIN_TRACE") && atoi(getenv("NFM_SEQ_WIN_TRACE")) != 0;
  a.n_fwd = n_fwd, a.n_res = n_res, a.terms = terms, a.ch = ch, a.wk = wk;
  a.W = W;
  a.lgW = lgW;
  a.no_cond = no_cond ? 1 : 0;
  a.first_worker = no_cond ? 0 : 1;
  a.one_term = one_term ? 1 : 0;
  a.par_min = 6;
  if (const char* env = getenv("NFM_SEQ_WIN_PAR")) a.par_min = atoi(env);
  a.np = np;
  const int thr = np - 1, near_r = W;
  a.thr = thr;
  a.near_r = near_r;
  a.m_cap = m_cap;
  a.FW = FW;
  a.lgKp = lgKp;
  const size_t lds_worker = win_worker_lds(wk, M, m_cap, ada, W);
  const size_t lds_cond = one_term ? sizeof(double) * (2 + 9 * (size_t)kSumRing) + sizeof(unsigned) * kSumRing : sizeof(double) * 2 + sizeof(ull) * (size_t)kWinRing * FW;
  size_t lds_bytes = lds_worker > lds_cond ? lds_worker : lds_cond;
  a.lds_worker = lds_worker, a.lds_cond = lds_cond;
  if (lds_bytes > 160 * 1024) return a.fallback = 2, a;
  if (lds_bytes < 81 * 1024) lds_bytes = 81 * 1024;
  a.lds_bytes = lds_bytes;
  a.ctl_zeroed = sizeof(unsigned) * (W + 64) + sizeof(double) * 2 * (W + 1);  // (the loop's memsets)
  a.fw_zeroed = sizeof(ull) * kFwSlot * np * (size_t)W;
  return a;
}

struct OneWg {  // which launch launch_sequential made: error 1 / 2 = its two NFM_CHECKs
  int error, pipe, staged, T, threads, S, lgS, rc_rung, split_terms, in_lds, m_cap;
  size_t lds_bytes, table_bytes;
};
static int pipe_rung(int rc, int threads) {  // launch_seq_pipe's ladders
  if (threads == kPipeThreadsWide) return rc <= 2 ? 2 : rc <= 4 ? 4 : rc <= 8 ? 8 : 16;
  return rc <= 1 ? 1 : rc <= 2 ? 2 : rc <= 4 ? 4 : rc <= 8 ? 8 : rc <= 16 ? 16 : rc <= 32 ? 32 : 64;
}
static void place_sample_table(int T, size_t table_bytes, size_t* lds_bytes, bool* global) {
  *global = false;
  *lds_bytes = sizeof(double) * (size_t)T + table_bytes;
  if (*lds_bytes <= 160 * 1024) return;
  *global = true;
  *lds_bytes = sizeof(double) * (size_t)T;
}
static OneWg launch_sequential(const ModelView& M, int m_cap, bool pipe_on, bool stage_on) {
  OneWg o{};
  if (!(M.Kp <= 1024)) return o.error = 1, o;
  if (!(M.kind == NFM_KIND_FFM || M.degree <= kSeqMaxDeg)) return o.error = 2, o;
  int T = ((M.Kp + kWave - 1) / kWave) * kWave;
  if (T < kWave) T = kWave;
  if (m_cap < 1) m_cap = 1;
  o.T = T, o.m_cap = m_cap, o.in_lds = 1;
  const bool ffm = M.kind == NFM_KIND_FFM;
  if (pipe_on && (ffm || (M.nb == 1 && M.degree == 2)) && M.nb >= 1 && M.nb < 32768 && m_cap <= kPipeThreads) {
    int S = 2, lgS = 1;
    while (S < M.Kp) { S <<= 1; ++lgS; }
    const int nbk = ffm ? M.nb : 1;
    const int64_t slots = (int64_t)nbk * m_cap;
    int threads = kPipeThreads;
    int G = S <= threads ? threads / S : 0;
    int64_t rc = G > 0 ? (slots + G - 1) / G : (int64_t)1 << 30;
    if (G > 0 && rc >= 8 && (slots + 2 * G - 1) / (2 * G) <= 16) {
      threads = kPipeThreadsWide;
      G *= 2;
      rc = (slots + G - 1) / G;
    }
    const size_t pair_doubles = ffm && (int64_t)m_cap * m_cap <= kPipePairCap ? (size_t)m_cap * m_cap : 0;
    const size_t base_doubles = (size_t)threads + 2 * (size_t)slots * S + 7 * (size_t)m_cap + pair_doubles;
    const size_t tail_bytes = sizeof(int64_t) * 3 * (size_t)m_cap +
                              sizeof(int) * ((size_t)m_cap + (ffm ? 3 * (size_t)m_cap + nbk + (size_t)nbk * m_cap : 0));
    const int split_terms = !ffm && sizeof(double) * (base_doubles + (size_t)m_cap * S) + tail_bytes <= 160 * 1024 ? 1 : 0;
    const size_t pipe_bytes = sizeof(double) * (base_doubles + (split_terms ? (size_t)m_cap * S : 0)) + tail_bytes;
    if (G >= 1 && rc <= 64 && pipe_bytes <= 160 * 1024) {
      o.pipe = 1, o.threads = threads, o.S = S, o.lgS = lgS, o.rc_rung = pipe_rung((int)rc, threads), o.split_terms = split_terms, o.lds_bytes = pipe_bytes;
      return o;
    }
  }
  const size_t n_da = (size_t)(M.nb > 0 ? M.nb : 1) * m_cap * T;
  size_t lds_bytes = 0;
  bool global = false;
  place_sample_table(T, sizeof(double) * n_da, &lds_bytes, &global);
  o.threads = T, o.in_lds = !global, o.table_bytes = sizeof(double) * n_da, o.lds_bytes = lds_bytes;
  if (M.kind == NFM_KIND_FFM) return o;
  const size_t staged_bytes = lds_bytes + sizeof(double) * (n_da + 3 * (size_t)m_cap);
  if (!global && stage_on && M.nb > 0 && staged_bytes <= 160 * 1024) {
    o.staged = 1, o.lds_bytes = staged_bytes;
    return o;
  }
  return o;
}
}  // namespace parent

// ---------------------------------------------------------------------------------------------------------------------------
static void put_env(const char* name, int v) {
  if (v == kKnobUnset) unsetenv(name);
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
  long long seen[8] = {0};  // supported, offered, offered and refused at the CUs, ... at the LDS, two-block, pipe, staged, scratch
  for (int draw = 0; draw < n; ++draw) {
    SeqShape S{};
    const int fam = (int)(rng() % 6);  // degree 2 | 65 ... 128 factors | wide rows | orders | field-aware | anything
    S.Kp = (int)pick({2, 4, 8, 16, 32, 64, 64, 64, 128});
    S.kind = SEQ_KIND_FM, S.degree = 2, S.nb = 1, S.kc = 1, S.d = pick({40, 1000, 100000}), S.n_aug = 0;
    if (fam == 1) S.Kp = 128;
    if (fam == 2) S.Kp = 128, S.nb = S.kc = (int)pick({2, 3, 8});
    if (fam == 3) S.degree = (int)pick({2, 3, 4, 6, 7, 8, 9}), S.nb = (int)pick({1, 2, 3, 5});
    if (fam == 4) S.kind = SEQ_KIND_FFM, S.nb = (int)pick({1, 2, 16, 39, 64});
    if (fam == 5) S.kind = (int)pick({0, 0, 1, 2}), S.degree = (int)pick({1, 2, 3}), S.nb = (int)pick({0, 1, 2}), S.n_aug = (int)pick({0, 0, 1}), S.kc = (int)pick({1, 1, 2});
    if (rng() % 16 == 0) {  // a four-wavefront worker a few hundred bytes below a CU's LDS at the workers the support check assumes
      S.kind = SEQ_KIND_FFM, S.degree = 2, S.Kp = 8, S.nb = 39, S.kc = 1, S.n_aug = 0;
    }
    const bool lds_edge = S.kind == SEQ_KIND_FFM && S.Kp == 8 && S.nb == 39 && rng() % 2;
    S.k = S.Kp, S.da = S.d + S.n_aug;
    const bool feature_major = fam == 2 || fam == 4 || (fam == 5 && rng() % 2);
    S.bs = feature_major ? 1 : S.da, S.rs = feature_major ? S.nb : 1;
    S.fit_intercept = (int)(rng() % 2), S.ada = (int)(rng() % 2);
    S.m_cap = (int)pick({0, 1, 2, 8, 16, 22, 23, 31, 32, 33, 39, 63, 64, 65, 100, 252, 253, 256, 257, 316, 317, 330, 1000});
    if (lds_edge) S.m_cap = 15, S.ada = 1, S.fit_intercept = 0;
    S.ns = pick({1, 2047, 2048, 100000, ((int64_t)1 << 31) - 1, (int64_t)1 << 31});
    S.nnz = pick({1000, ((int64_t)1 << 32) - 1, (int64_t)1 << 32, 1000, 1000});
    if (rng() % 16 == 0) S.d = pick({((int64_t)1 << 31) - 1, (int64_t)1 << 31});
    S.n_cu = (int)pick({16, 17, 64, 65, 128, 129, 256, 257, 304});
    SeqKnobs K;
    K.win = (int)pick({kKnobUnset, kKnobUnset, 0, 1, 2, 2, 2, 2});
    K.exact = (int)pick({kKnobUnset, kKnobUnset, 0, 1});
    K.nocond = (int)pick({kKnobUnset, kKnobUnset, 0, 1});
    K.w = (int)pick({kKnobUnset, kKnobUnset, kKnobUnset, 1, 8, 16, 100, 128, 256, 1000});
    K.par = (int)pick({kKnobUnset, 0, 6, 9});
    K.trace = (int)pick({kKnobUnset, 0, 1});
    K.pipe = (int)pick({kKnobUnset, kKnobUnset, 0, 1});
    K.stage = (int)pick({kKnobUnset, kKnobUnset, 0, 1});
    const int64_t fallbacks = pick({0, 0, 1, 2, 3});
    const bool have_seqwin = fallbacks > 0 || rng() % 2;
    const size_t snap_bytes = (size_t)pick({0, 1000000, 819200000, 819200001, (long long)(S.ns < 1000000 ? S.ns * 400000 : 0), 520000000});
    put_env("NFM_SEQ_WIN", K.win), put_env("NFM_SEQ_WIN_EXACT", K.exact), put_env("NFM_SEQ_WIN_NOCOND", K.nocond);
    put_env("NFM_SEQ_WIN_W", K.w), put_env("NFM_SEQ_WIN_PAR", K.par), put_env("NFM_SEQ_WIN_TRACE", K.trace);
    {  // seq_knobs() reads what was just set (the per-call variables)
      const SeqKnobs e = seq_knobs();
      SAME("knobs", e.win == K.win && e.exact == K.exact && e.nocond == K.nocond && e.w == K.w && e.par == K.par && e.trace == K.trace, 1);
    }
    const parent::ModelView M{S.d, S.da, S.nb, S.k, S.Kp, S.Kp / 2, S.degree, S.n_aug, S.kind, S.fit_intercept, S.kc, S.bs, S.rs};
    // ---- the window ----
    const WinRoute r = win_route(S, K, fallbacks, snap_bytes);
    const parent::ModelView Mw = parent::seq_window_view(M);
    SAME("two_block", r.two_block, Mw.Kp != M.Kp);
    SAME("view nb", r.nb, Mw.nb);
    SAME("view Kp", r.Kp, Mw.Kp);
    SAME("supported", r.supported, parent::seq_window_supported(Mw, S.m_cap, S.ns, S.nnz, S.n_cu, S.ada != 0));
    SAME("offered", r.offered, parent::seq_window_offered(Mw, S.m_cap, S.ns, S.nnz, S.n_cu, S.ada != 0, have_seqwin, fallbacks, snap_bytes));
    seen[0] += r.supported, seen[1] += r.offered, seen[4] += r.two_block && r.supported;
    if (r.supported) {  // (the parent's launcher ran for offered calls only; its lines do not depend on the offer)
      const parent::Launch a = parent::launch_sequential_window(S.n_cu, S.ada != 0, Mw, S.ns, S.m_cap, fallbacks);
      SAME("fits_cus", r.fits_cus, a.fallback != 1);
      SAME("fits", r.fits, a.fallback == 0);
      seen[2] += r.offered && a.fallback == 1, seen[3] += r.offered && a.fallback == 2;
      if (a.fallback != 1) {
        SAME("W", r.W, a.W); SAME("lgW", r.lgW, a.lgW); SAME("no_cond", r.no_cond, a.no_cond); SAME("first_worker", r.first_worker, a.first_worker);
        SAME("one_term", r.one_term, a.one_term); SAME("par_min", r.par_min, a.par_min); SAME("np", r.np, a.np); SAME("thr", r.thr, a.thr);
        SAME("near_r", r.near_r, a.near_r); SAME("m_cap", r.m_cap, a.m_cap); SAME("FW", r.FW, a.FW); SAME("lgKp", r.lgKp, a.lgKp);
        SAME("ch", r.ch, a.ch); SAME("wk", r.wk, a.wk); SAME("terms", r.terms, a.terms); SAME("trace", K.trace != kKnobUnset && K.trace != 0, a.trace);
        SAME("n_fwd", r.n_fwd, a.n_fwd); SAME("n_res", r.n_res, a.n_res); SAME("mail bytes", 8 * (r.n_fwd + r.n_res), a.mail_bytes);
        SAME("ctl bytes", 4 * r.n_ctl + 8 * r.n_partial + 16, a.ctl_bytes); SAME("scales bytes", 8 * r.n_scales, a.scales_bytes);
        SAME("fw bytes", 8 * r.n_fw, a.fw_bytes); SAME("lds_worker", r.lds_worker, a.lds_worker); SAME("lds_cond", r.lds_cond, a.lds_cond);
      }
      if (a.fallback == 0) {
        SAME("lds_bytes", r.lds_bytes, a.lds_bytes); SAME("ctl zeroed", 4 * r.n_ctl + 8 * r.n_partial, a.ctl_zeroed);
        SAME("fw zeroed", 8 * r.n_fw_tags, a.fw_zeroed);
      }
    }
    // ---- one workgroup: the same numbers taken as the model seq_row_view hands over, with rows of up to 1025 doubles ----
    SeqShape R = S;
    if (rng() % 3 == 0) R.Kp = R.k = (int)pick({192, 256, 320, 512, 1000, 1024, 1025});
    const parent::ModelView Mr{R.d, R.da, R.nb, R.k, R.Kp, 64, R.degree, R.n_aug, R.kind, R.fit_intercept, R.kc, R.bs, R.rs};
    const SeqOneWg w = seq_one_wg_route(R, K);
    const parent::OneWg p = parent::launch_sequential(Mr, R.m_cap, K.pipe != 0, K.stage != 0);
    SAME("refusal", w.refusal, p.error);
    if (!p.error) {
      SAME("pipe", w.step == SEQ_PIPE, p.pipe); SAME("staged", w.step == SEQ_STAGED, p.staged); SAME("T", w.T, p.T); SAME("threads", w.threads, p.threads);
      SAME("S", w.S, p.S); SAME("lgS", w.lgS, p.lgS); SAME("rc", w.rc, p.rc_rung); SAME("split_terms", w.split_terms, p.split_terms);
      SAME("one-wg lds", w.lds_bytes, p.lds_bytes); SAME("table_in_lds", w.table_in_lds, p.in_lds); SAME("table_bytes", w.table_bytes, p.table_bytes);
      SAME("one-wg m_cap", w.m_cap, p.m_cap);
      seen[5] += p.pipe, seen[6] += p.staged, seen[7] += !p.in_lds;
    }
  }
  printf("draws %d disagreements %lld | supported %lld offered %lld refused_cus %lld refused_lds %lld two_block %lld | pipe %lld staged %lld scratch %lld\n", n,
         n_bad, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5], seen[6], seen[7]);
  return n_bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "knobs") == 0) {
    const SeqKnobs k = seq_knobs();
    printf("%d %d %d %d %d %d %d %d %s\n", k.win, k.exact, k.nocond, k.w, k.par, k.trace, k.pipe, k.stage, k.trace_file ? k.trace_file : "-");
    return 0;
  }
  if (argc > 3 && strcmp(argv[1], "parent") == 0) return parent_draws(atoi(argv[2]), (unsigned)atoi(argv[3]));
  long long n_lines = 0;
  for (;;) {
    SeqShape S{};
    SeqKnobs K;
    long long d, da, bs, rs, ns, nnz, fallbacks;
    unsigned long long snap;
    const int got = scanf("%d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %lld %lld %d %d %d %d %d %d %d %d %d %d %lld %llu", &S.kind, &S.degree, &S.nb, &S.kc,
                          &S.k, &S.Kp, &S.n_aug, &S.fit_intercept, &d, &da, &bs, &rs, &S.m_cap, &ns, &nnz, &S.ada, &S.n_cu, &K.win, &K.exact, &K.nocond,
                          &K.w, &K.par, &K.trace, &K.pipe, &K.stage, &fallbacks, &snap);
    if (got == EOF) break;
    if (got != 27) {
      fprintf(stderr, "line %lld: %d of 27 fields\n", n_lines + 1, got);
      return 2;
    }
    S.d = d, S.da = da, S.bs = bs, S.rs = rs, S.ns = ns, S.nnz = nnz;
    const WinRoute r = win_route(S, K, fallbacks, (size_t)snap);
    const SeqOneWg w = seq_one_wg_route(S, K);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %s | ", r.two_block, r.nb, r.Kp,
           r.supported, r.reason, r.offered, r.no_cond, r.one_term, r.wk, r.W, r.lgW, r.first_worker, r.m_cap, r.lgKp, r.terms, r.ch, r.FW, r.np, r.thr,
           r.near_r, r.par_min, r.lds_worker, r.lds_cond, r.lds_bytes, r.n_fwd, r.n_res, r.n_ctl, r.n_partial, r.n_fw, r.n_fw_tags, r.n_scales,
           r.fits_cus, r.fits, r.counter[0] ? r.counter : "-");
    printf("%d %d %d %d %d %d %d %d %d %zu %d %zu %s\n", w.refusal, w.step, w.m_cap, w.T, w.threads, w.S, w.lgS, w.rc, w.split_terms, w.lds_bytes,
           w.table_in_lds, w.table_bytes, w.counter[0] ? w.counter : "-");
    ++n_lines;
  }
  fprintf(stderr, "seq_route: %lld cases\n", n_lines);
  return 0;
}
