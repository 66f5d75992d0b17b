// tests/cpp/mb_ffm_route_test.cpp -- nimfm_amd/csrc/mb_ffm_route.h as a filter: one case per line on stdin; its row kernel, LDS
// layout, route and work bounds per line on stdout.  tests/test_cpp_mb_ffm_route.py feeds it the cases of
// tests/ffm_kernel_cases.py and compares with their restatements.  Host only: no HIP, no library (g++ -std=c++17; a second build
// with -fsanitize=address,undefined runs the same cases).  With the argument "knobs": what ffm_knobs() reads from the environment.
//
// in:  L opt nb Kp max_row first_singleton | lds refresh (-2147483648 = unset) | b len uniq touches heavy segs |
//      max_batch max_unique max_touch max_heavy max_segs   (without the bars)
// out: kernel lds_bytes wpb raise_lds_limit m_cap counter | rows fmask xs js fs per_wave (ffm_row_lds of m_cap, nb, Kp) |
//      refresh use_stored nA nR nB nsb nH off_refresh off_col off_heavy n_parts | contrib rec partsA partsB hpart |
//      kFfmLdsShare kFfmLdsDefault the big counter's name
#include <stdio.h>
#include <string.h>

#include "../../nimfm_amd/csrc/mb_ffm_route.h"

using namespace nfm;

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "knobs") == 0) {
    const FfmKnobs k = ffm_knobs();
    printf("%d %d\n", k.lds, k.refresh);
    return 0;
  }
  long long n_lines = 0;
  for (;;) {
    FfmShape S{};
    FfmKnobs K;
    FfmBatch B{};
    long long b, uniq, touches, heavy, segs, max_batch, max_unique, max_touch, max_heavy, max_segs;
    const int got = scanf("%d %d %d %d %d %d %d %d %lld %d %lld %lld %lld %lld %lld %lld %lld %lld %lld", &S.L, &S.opt, &S.nb, &S.Kp, &S.max_row,
                          &S.first_singleton, &K.lds, &K.refresh, &b, &B.len, &uniq, &touches, &heavy, &segs, &max_batch, &max_unique,
                          &max_touch, &max_heavy, &max_segs);
    if (got == EOF) break;
    if (got != 19) {
      fprintf(stderr, "line %lld: %d of 19 fields\n", n_lines + 1, got);
      return 2;
    }
    B.b = b, B.uniq = uniq, B.touches = touches, B.heavy = heavy, B.segs = segs;
    const FfmRow row = ffm_row_kernel(S, K);
    const FfmRowLds l = ffm_row_lds(row.m_cap, S.nb, S.Kp);
    const FfmRoute r = ffm_route(S, K, row, B);
    const FfmBounds w = ffm_work_bounds(S, row, max_batch, max_unique, max_touch, max_heavy, max_segs);
    printf("%d %zu %d %d %d %s | %zu %zu %zu %zu %zu %zu | %d %d %d %d %d %d %d %d %d %d %d | %lld %lld %lld %lld %lld | %zu %zu %s\n", row.kernel,
           row.lds_bytes, row.wpb, row.raise_lds_limit, row.m_cap, row.counter, l.rows, l.fmask, l.xs, l.js, l.fs, l.per_wave, r.refresh,
           r.use_stored, r.nA, r.nR, r.nB, r.nsb, r.nH, r.off_refresh, r.off_col, r.off_heavy, r.n_parts, (long long)w.contrib, (long long)w.rec,
           (long long)w.partsA, (long long)w.partsB, (long long)w.hpart, kFfmLdsShare, kFfmLdsDefault, kFfmRowBigCounter);
    ++n_lines;
  }
  fprintf(stderr, "mb_ffm_route: %lld cases\n", n_lines);
  return 0;
}
