// tests/cpp/seqwin_layout_test.cpp -- nimfm_amd/csrc/seqwin_layout.h against the four byte-count formulas the host used to
// restate by hand (win_ffm_lds, win_fmx_lds, and the general / register-resident workers' formulas inline in
// seq_window_supported and launch_sequential_window), over a grid of shapes; and the carve-ups themselves: no array
// overlaps the next, the last one ends inside the request, 8-byte arrays start 8-byte aligned.  Host only: no HIP, no library.
// This checks the header against the host's earlier counts and against itself; it cannot see the three kernels that still
// carve their LDS by hand (win_worker, win_worker_ffm, win_worker_fmx).
#include <stdio.h>

#include "../../nimfm_amd/csrc/seqwin_layout.h"

using namespace nfm;

// ---- the formulas as they stood (kWave = 64, kFfmWaves = 4, dev::kMaxDeg = 6) ----
static const int kWave = 64, kFfmWaves = 4, kMaxDeg = 6;
typedef unsigned long long ull;

static size_t old_ffm_lds(int Kp, int nb, int m_cap, bool ada, int W) {
  int lgKp = 1;
  while ((1 << lgKp) < Kp) ++lgKp;
  const int grp = (kWave >> lgKp) * 4;
  const size_t mcs = ((size_t)m_cap * nb + grp - 1) / grp * grp;
  return sizeof(double) * ((ada ? 4 : 2) * mcs * Kp + (size_t)m_cap * m_cap + 4 * kWave + kFfmWaves + (ada ? 4 : 2) * (size_t)m_cap) +
         sizeof(ull) * 2 + sizeof(int) * (5 * (size_t)m_cap + nb + (size_t)nb * m_cap) + sizeof(unsigned) * W + 64;
}
static size_t old_fmx_lds(int Kp, int nb, int m_cap, bool ada, int W) {
  int lgKp = 1;
  while ((1 << lgKp) < Kp) ++lgKp;
  const int grp = (kWave >> lgKp) * 4;
  const size_t mcs = ((size_t)m_cap * nb + grp - 1) / grp * grp;
  return sizeof(double) * ((ada ? 4 : 2) * mcs * Kp + kWave + 4 * kWave + 3 * kMaxDeg * kWave + kFfmWaves + (ada ? 4 : 2) * (size_t)m_cap) +
         sizeof(ull) * 3 + sizeof(int) * 4 * (size_t)m_cap + sizeof(unsigned) * W + 64;
}
static size_t old_general_lds(int Kp, int m_cap, bool ada, int W) {
  int lgKp = 1;
  while ((1 << lgKp) < Kp) ++lgKp;
  const int grp = (kWave >> lgKp) * 4;
  const size_t mcp = (size_t)(m_cap + grp - 1) / grp * grp;
  const size_t rows = mcp * Kp;
  return sizeof(double) * ((ada ? 4 : 2) * rows + kWave + (ada ? 4 : 2) * mcp) + sizeof(int) * 3 * mcp + sizeof(unsigned) * W;
}
static size_t old_k64_lds(bool ada, int W) {
  return sizeof(double) * ((ada ? 3 : 1) * (size_t)kWave * kWave + kWave) + sizeof(unsigned) * W;
}

static int failures = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      if (failures++ < 20) {      \
        printf("FAIL: " __VA_ARGS__); \
        printf("\n");             \
      }                           \
    }                             \
  } while (0)

template <int N>
static void check_arrays(const WinLds<N>& L, size_t slack, const char* who, const WinShape& s) {
  size_t end = 0;
  for (int i = 0; i < N; ++i) {
    const WinLdsArray& a = L.a[i];
    CHECK(a.elem == 4 || a.elem == 8, "%s array %d: element of %d bytes", who, i, a.elem);
    CHECK(a.off >= end, "%s array %d starts at %zu, inside its predecessor (ends at %zu) Kp=%d nb=%d m_cap=%d ada=%d W=%d", who, i, a.off, end, s.Kp,
          s.nb, s.m_cap, (int)s.ada, s.W);
    if (a.elem == 8) CHECK(a.off % 8 == 0, "%s array %d: 8-byte elements at offset %zu", who, i, a.off);
    CHECK(a.off % 4 == 0, "%s array %d: offset %zu", who, i, a.off);
    end = a.off + a.bytes;
  }
  CHECK(end + slack == L.total, "%s: the last array ends at %zu, the request is %zu (slack %zu)", who, end, L.total, slack);
  CHECK(end <= L.total, "%s: the last array ends at %zu, beyond the request of %zu", who, end, L.total);
}

int main() {
  const int Kps[] = {2, 4, 8, 16, 32, 64}, nbs[] = {1, 2, 5, 16, 39}, mcaps[] = {1, 2, 7, 16, 33, 64, 316}, Ws[] = {16, 64, 128, 256};
  long shapes = 0;
  for (int Kp : Kps)
    for (int nb : nbs)
      for (int m_cap : mcaps)
        for (int ada = 0; ada < 2; ++ada)
          for (int W : Ws) {
            const WinShape s{Kp, win_lg(Kp), nb, /*k=*/Kp, m_cap, ada != 0, W};
            const auto G = win_general_lds(s);
            const auto K = win_k64_lds(s);
            const auto F = win_slots_lds(s, true);
            const auto X = win_slots_lds(s, false);
            CHECK(G.total == old_general_lds(Kp, m_cap, ada, W), "general: %zu != %zu (Kp=%d m_cap=%d ada=%d W=%d)", G.total,
                  old_general_lds(Kp, m_cap, ada, W), Kp, m_cap, ada, W);
            CHECK(K.total == old_k64_lds(ada, W), "k64: %zu != %zu (ada=%d W=%d)", K.total, old_k64_lds(ada, W), ada, W);
            CHECK(F.total == old_ffm_lds(Kp, nb, m_cap, ada, W), "field-aware: %zu != %zu (Kp=%d nb=%d m_cap=%d ada=%d W=%d)", F.total,
                  old_ffm_lds(Kp, nb, m_cap, ada, W), Kp, nb, m_cap, ada, W);
            CHECK(X.total == old_fmx_lds(Kp, nb, m_cap, ada, W), "orders: %zu != %zu (Kp=%d nb=%d m_cap=%d ada=%d W=%d)", X.total,
                  old_fmx_lds(Kp, nb, m_cap, ada, W), Kp, nb, m_cap, ada, W);
            check_arrays(G, 0, "general", s);
            check_arrays(K, 0, "k64", s);
            check_arrays(F, kWinLdsSlotsSlack, "field-aware", s);
            check_arrays(X, kWinLdsSlotsSlack, "orders", s);
            ++shapes;
          }
  // what seq_window_supported assumes for W
  CHECK(kWinLdsSupportW == 256 && kWinLdsSupportWSlots == 128, "the worker counts seq_window_supported assumes");
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("seqwin layout ok (%ld shapes)\n", shapes);
  return 0;
}
