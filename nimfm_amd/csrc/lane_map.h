// nimfm_amd/csrc/lane_map.h -- how many row slots a sample gets on a 64-lane wavefront (choose_split), for the mini-batch row
// phase and decisionFunction.  Plain C++: no HIP header, so the host-only header mb_route.h and its g++ test see the same text as
// the library.  common.h's kWave, kBlock and kWavesPerBlock are restated here under names of their own, as seqwin_layout.h does,
// and common.h asserts that they agree.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace nfm {

constexpr int kLaneWave = 64;   // common.h: kWave
constexpr int kLaneBlock = 256;  // common.h: kBlock, 4 waves per workgroup
constexpr int kLaneWavesPerBlock = kLaneBlock / kLaneWave;

// SPLIT (row slots per sample, fm_device.h) for a launch over n samples with avg_row nnz per row:
// enough wavefronts to fill the chip (>= 16 per CU) and a serial chain of at most ~8 rounds of
// kUnroll loads per lane (measured on cfg2: fewer slots win as soon as the chip is full); capped by the 64/L slots a wavefront has and by 16.
inline int choose_split(int L, int64_t n, double avg_row, int n_cu) {
  const int R = kLaneWave / L;
  auto p2 = [](double v) {
    int r = 1;
    while (r < v && r < 64) r <<= 1;
    return r;
  };
  if (const char* env = getenv("NFM_SPLIT")) {  // tuning override
    int s = atoi(env);
    if (s >= 1) return s > R ? R : (s > 16 ? 16 : p2(s));
  }
  const double occ = (double)n_cu * 16.0 * kLaneWave / ((double)(n > 0 ? n : 1) * L);
  int s = p2(occ);
  const int lat = p2(avg_row / 32.0);
  if (lat > s) s = lat;
  if (s > R) s = R;
  if (s > 16) s = 16;
  return s < 1 ? 1 : s;
}

}  // namespace nfm
