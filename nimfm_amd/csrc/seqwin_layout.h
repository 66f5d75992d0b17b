// nimfm_amd/csrc/seqwin_layout.h -- the LDS carve-up of the dependency window's four workers (seqwin.hip): every array's
// offset and the bytes to request.  The host takes ALL its byte counts from here (win_route, seq_route.h: the support check and
// the launch's request); of the kernels only win_worker_k64 takes its pointers from here so far -- win_worker,
// win_worker_ffm and win_worker_fmx still carve the same layout by hand (seqwin.hip's header says why), so for these three a
// carve-up exists twice and nothing checks the kernel's copy against this one: a change to one of them goes into both.
// (A host count that fell short of a kernel's pointer arithmetic would let the kernel write past its LDS request.)
// Plain C++, integers only: tests/cpp/seqwin_layout_test.cpp builds it with g++ and holds its totals against the host's
// earlier formulas, and its arrays against overlap, overrun and misalignment.
#ifndef NIMFM_SEQWIN_LAYOUT_H
#define NIMFM_SEQWIN_LAYOUT_H
#include <stddef.h>

#if defined(__HIPCC__)
#define NFM_WINLDS_FN __host__ __device__ inline
#else
#define NFM_WINLDS_FN inline
#endif

namespace nfm {

constexpr int kWinLdsWave = 64;     // lanes of a wavefront (common.h: kWave)
constexpr int kWinLdsWaves = 4;     // wavefronts of a four-wavefront worker (seqwin.hip: kFfmWaves)
constexpr int kWinLdsMaxDeg = 6;    // highest degree of an order (fm_device.h: dev::kMaxDeg)
constexpr int kWinLdsSupportW = 256;  // the worker count win_route's support check assumes for the one-wavefront workers' counters ...
constexpr int kWinLdsSupportWSlots = 128;  // ... and for the four-wavefront workers' (the most their launches use)

struct WinShape {
  int Kp, lgKp;          // lanes per row (a power of two >= 2) and its logarithm: win_lg(Kp), WinArgs::lgKp in the kernels
  int nb, k, m_cap;      // blocks (fields / orders), factors, longest row.  (No array depends on k: rows are padded to Kp.)
  bool ada;              // AdaGrad: g_sum / g_norm beside every row and linear weight
  int W;                 // workers: one completion counter each
};

struct WinLdsArray {
  size_t off, bytes;  // from the start of the workgroup's dynamic LDS
  int elem;           // bytes per element
};

template <int N>
struct WinLds {
  WinLdsArray a[N];  // in address order; an array the flavour does not have: 0 bytes
  size_t total;      // bytes to request for the worker
  template <class T>
  NFM_WINLDS_FN T* ptr(void* lds, int which) const {
    return reinterpret_cast<T*>(static_cast<char*>(lds) + a[which].off);
  }
};

// a[which] = `count` elements of `elem` bytes behind everything laid out so far
template <int N>
NFM_WINLDS_FN void win_lds_put(WinLds<N>& L, int which, size_t count, int elem) {
  L.a[which].off = L.total;
  L.a[which].bytes = count * (size_t)elem;
  L.a[which].elem = elem;
  L.total += count * (size_t)elem;
}

inline int win_lg(int Kp) {  // (host: the launcher's lgKp)
  int lgKp = 1;
  while ((1 << lgKp) < Kp) ++lgKp;
  return lgKp;
}
// rows are handled (64 / Kp) * 4 at a time without a branch per row: the per-sample arrays are padded to whole groups
NFM_WINLDS_FN size_t win_lds_padded(int lgKp, size_t rows) {
  const int lg = 8 - lgKp;  // the group: (64 >> lgKp) * 4 rows, a power of two (a shift, not a 64-bit division, in the kernels)
  return (rows + ((size_t)1 << lg) - 1) >> lg << lg;
}

// ---- win_worker: degree 2, any row shape, the sample's rows in LDS ----
enum { WG_Pl, WG_Tl, WG_Gl, WG_Nl, WG_red, WG_vl, WG_wl, WG_gwl, WG_nwl, WG_jl, WG_pl, WG_ll, WG_cnt, WG_N };
NFM_WINLDS_FN WinLds<WG_N> win_general_lds(const WinShape& s) {
  WinLds<WG_N> L{};
  const size_t mc = win_lds_padded(s.lgKp, (size_t)s.m_cap), ada = s.ada ? 1 : 0;
  win_lds_put(L, WG_Pl, mc * s.Kp, 8);         // [mc][Kp] stored parameter values of the sample's rows
  win_lds_put(L, WG_Tl, mc * s.Kp, 8);         // [mc][Kp] x_q p_qs, then the derivative
  win_lds_put(L, WG_Gl, ada * mc * s.Kp, 8);   // AdaGrad: [mc][Kp] g_sum
  win_lds_put(L, WG_Nl, ada * mc * s.Kp, 8);   // AdaGrad: [mc][Kp] g_norm
  win_lds_put(L, WG_red, kWinLdsWave, 8);      // [64]
  win_lds_put(L, WG_vl, mc, 8);                // [mc] values
  win_lds_put(L, WG_wl, mc, 8);                // [mc] stored linear weights (AdaGrad: after update())
  win_lds_put(L, WG_gwl, ada * mc, 8);         // AdaGrad: [mc] g_sum of the linear term
  win_lds_put(L, WG_nwl, ada * mc, 8);         // AdaGrad: [mc] g_norm
  win_lds_put(L, WG_jl, mc, 4);                // [mc] feature ids
  win_lds_put(L, WG_pl, mc, 4);                // [mc] previous position with the same feature
  win_lds_put(L, WG_ll, mc, 4);                // [mc] 1: the row comes from its writer's recipe, not from memory
  win_lds_put(L, WG_cnt, (size_t)s.W, 4);      // [W] completion counters as last seen
  return L;
}

// ---- win_worker_k64: rows of 64 factors, at most 64 entries, the sample's rows in registers ----
enum { WK64_Fl, WK64_Gl, WK64_Nl, WK64_red, WK64_cnt, WK64_N };
NFM_WINLDS_FN WinLds<WK64_N> win_k64_lds(const WinShape& s) {
  WinLds<WK64_N> L{};
  const size_t K = kWinLdsWave, ada = s.ada ? 1 : 0;
  win_lds_put(L, WK64_Fl, K * K, 8);           // [64][64] rows that arrived late (forwarded or read again)
  win_lds_put(L, WK64_Gl, ada * K * K, 8);     // AdaGrad: [64][64] g_sum of the sample's rows
  win_lds_put(L, WK64_Nl, ada * K * K, 8);     // AdaGrad: [64][64] g_norm
  win_lds_put(L, WK64_red, K, 8);              // [64]
  win_lds_put(L, WK64_cnt, (size_t)s.W, 4);    // [W] completion counters as last seen
  return L;
}

// ---- win_worker_ffm / win_worker_fmx: four wavefronts, a sample's rows are its slots (entry, field) / (entry, order) ----
enum {
  WS_Pl, WS_Tl, WS_Gl, WS_Nl, WS_pc, WS_red, WS_bc, WS_affB, WS_affP, WS_affD, WS_vsum, WS_vl, WS_wl, WS_gwl, WS_nwl,
  WS_mk, WS_jl, WS_fl, WS_pl, WS_ql, WS_ll, WS_fcnt, WS_fent, WS_cnt, WS_N
};
constexpr size_t kWinLdsSlotsSlack = 64;  // bytes requested beyond the last array
NFM_WINLDS_FN WinLds<WS_N> win_slots_lds(const WinShape& s, bool ffm) {
  WinLds<WS_N> L{};
  const size_t mcap = (size_t)s.m_cap, F = (size_t)s.nb, ada = s.ada ? 1 : 0, f = ffm ? 1 : 0, x = ffm ? 0 : 1;
  const size_t mcs = win_lds_padded(s.lgKp, mcap * F);  // slots, padded to whole groups
  const size_t DW = (size_t)kWinLdsMaxDeg * kWinLdsWave;
  win_lds_put(L, WS_Pl, mcs * s.Kp, 8);        // [mcs][Kp] stored parameter values of the sample's slots
  win_lds_put(L, WS_Tl, mcs * s.Kp, 8);        // [mcs][Kp] the slots' derivative
  win_lds_put(L, WS_Gl, ada * mcs * s.Kp, 8);  // AdaGrad: g_sum
  win_lds_put(L, WS_Nl, ada * mcs * s.Kp, 8);  // AdaGrad: g_norm
  win_lds_put(L, WS_pc, f * mcap * mcap, 8);   // field-aware: [mcap][mcap] the pairs' terms of the prediction
  win_lds_put(L, WS_red, x * kWinLdsWave, 8);  // orders: [64] an order's kernel per factor
  win_lds_put(L, WS_bc, 4 * kWinLdsWave, 8);   // [4][64] per near entry: the writer's dL, scale, step size, next scale
  win_lds_put(L, WS_affB, x * DW, 8);          // orders: [DG][64] the affine entry's rows: slope in its writer's dL, per order
  win_lds_put(L, WS_affP, x * DW, 8);          // orders: [DG][64] ... the rows as the writer used them, and
  win_lds_put(L, WS_affD, x * DW, 8);          // orders: [DG][64] ... their derivatives (the recipe, kept for the exact rows)
  win_lds_put(L, WS_vsum, kWinLdsWaves, 8);    // [NW] the wavefronts' viol
  win_lds_put(L, WS_vl, mcap, 8);              // [mcap] values
  win_lds_put(L, WS_wl, mcap, 8);              // [mcap] stored linear weights (AdaGrad: after update())
  win_lds_put(L, WS_gwl, ada * mcap, 8);       // AdaGrad: [mcap]
  win_lds_put(L, WS_nwl, ada * mcap, 8);       // AdaGrad: [mcap]
  win_lds_put(L, WS_mk, ffm ? 2 : 3, 8);       // {near entries, hot entries} of the sample; orders: + {affine entry + 1}
  win_lds_put(L, WS_jl, mcap, 4);              // [mcap] feature ids
  win_lds_put(L, WS_fl, f * mcap, 4);          // field-aware: [mcap] fields
  win_lds_put(L, WS_pl, mcap, 4);              // [mcap] previous position with the same feature
  win_lds_put(L, WS_ql, mcap, 4);              // [mcap] the feature's entry index in that sample
  win_lds_put(L, WS_ll, mcap, 4);              // [mcap] 1: the entry's rows come from their writer's recipe
  win_lds_put(L, WS_fcnt, f * F, 4);           // field-aware: [F] entries of the sample per field
  win_lds_put(L, WS_fent, f * F * mcap, 4);    // field-aware: [F][mcap] ... which ones, ascending
  win_lds_put(L, WS_cnt, (size_t)s.W, 4);      // [W] completion counters as last seen (wavefront 0's)
  L.total += kWinLdsSlotsSlack;
  return L;
}

}  // namespace nfm
#endif
