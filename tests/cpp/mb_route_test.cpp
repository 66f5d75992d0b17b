// tests/cpp/mb_route_test.cpp -- nimfm_amd/csrc/mb_route.h as a filter: one case per line on stdin, its route and the work
// bounds per line on stdout.  tests/test_cpp_mb_route.py feeds it the cases of tests/row_slot_cases.py and tests/mb_route_cases.py
// and compares with their restatements.  Host only: no HIP, no library (g++ -std=c++17; a second build with
// -fsanitize=address,undefined runs the same cases).
//
// in:  split_request (0 = NFM_SPLIT unset) |
//      L opt gen nb n_aug fit_linear d max_row avg_row n_cu use_singles first_singleton rows_ascend table_bytes compact_sched col_occ |
//      the fifteen knobs in MbKnobs' order (-2147483648 = unset) | b len uniq touches heavy segs
// out: use_stored row_kernel slots mode sing stream_rows nA singles_in_row singles_in_col nS stage_w w_cap w_parts w_wg w_slice
//      bad_passes stage_dl dl_grid col_kernel nB nsb nH | held_entries held_capacity (of L and the route's slots) |
//      partsA partsB dLt Wt (mb_work_bounds with the batch's own numbers as the plan's maxima) | the two counters' names
#include <inttypes.h>
#include <stdio.h>

#include "../../nimfm_amd/csrc/mb_route.h"

using namespace nfm;

int main() {
  long long n_lines = 0;
  for (;;) {
    int request;
    MbShape S{};
    MbKnobs K;
    MbBatch B{};
    long long d, table_bytes, b, uniq, touches, heavy, segs;
    const int got = scanf("%d %d %d %d %d %d %d %lld %d %lf %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %d %lld %lld %lld %lld",
                          &request, &S.L, &S.opt, &S.gen, &S.nb, &S.n_aug, &S.fit_linear, &d, &S.max_row, &S.avg_row, &S.n_cu, &S.use_singles,
                          &S.first_singleton, &S.rows_ascend, &table_bytes, &S.compact_sched, &S.col_occ, &K.tu, &K.col_long,
                          &K.col_long_compact, &K.stage_dl, &K.stage_w, &K.stage_w_passes, &K.col_grid, &K.stream, &K.singles_kernel, &K.held,
                          &K.nq, &K.col_pipe, &K.col_wg, &K.col_cap_sets, &K.ada2, &b, &B.len, &uniq, &touches, &heavy, &segs);
    if (got == EOF) break;
    if (got != 38) {
      fprintf(stderr, "line %lld: %d of 38 fields\n", n_lines + 1, got);
      return 2;
    }
    S.d = d, S.table_bytes = (uint64_t)table_bytes;
    B.b = b, B.uniq = uniq, B.touches = touches, B.heavy = heavy, B.segs = segs;
    if (request > 0) {
      char buf[16];
      snprintf(buf, sizeof buf, "%d", request);
      setenv("NFM_SPLIT", buf, 1);
    } else {
      unsetenv("NFM_SPLIT");
    }
    const MbRoute r = mb_route(S, K, B);
    const MbBounds w = mb_work_bounds(S, K, B.len, B.uniq, B.touches, B.heavy);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %" PRId64 " %d %d %d %d %d %d %d | %d %d | %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " | %s %s\n",
           r.use_stored, r.row_kernel, r.slots, r.mode, r.sing, r.stream_rows, r.nA, r.singles_in_row, r.singles_in_col, r.nS, r.stage_w,
           r.w_cap, r.w_parts, r.w_wg, r.w_slice, r.bad_passes, r.stage_dl, r.dl_grid, r.col_kernel, r.nB, r.nsb, r.nH,
           held_entries(S.L, r.slots), held_capacity(S.L, r.slots), w.partsA, w.partsB, w.dLt, w.Wt, mb_row_counter(r), mb_col_counter(r));
    ++n_lines;
  }
  fprintf(stderr, "mb_route: %lld cases\n", n_lines);
  return 0;
}
