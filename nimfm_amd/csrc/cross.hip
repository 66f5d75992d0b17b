// nimfm_amd/csrc/cross.hip -- crossDecisionFunction and the top K of every row of it (cross.h).
//
// The reference scores the rows it is given (model/factorization_machine.nim:100-122): ranking all items for a user means
// one row per (user, item) pair, hstack(U[rep], V[tile]) (tensor/sparse.nim:671-698).  The degree-2 kernel
// (kernels.nim:59-64) factorises over the two halves of such a row, so the pairs are never made:
//   k_cross_side    per row of U and of V: the Kq sums q_s and the row's own scalar (fm_device.h's lane mapping, the
//                   storage order of the row, the ascending factor sum of k_fm_predict)
//   cross_tile      a kCrossTU x kCrossTV block of sum_s q_us q_vs on v_mfma_f64_16x16x4_f64, the factors in one fixed order
//   k_cross_scores  the tile over a 2-D grid -> out[nU][nV]
//   k_cross_topk    the tile over (user tile, item chunk): the K best of the chunk per user, kept sorted in LDS
//   k_cross_merge   the chunks' lists -> the K best per user
//   k_cross_topk<true>   the same with a seen matrix: per user a cursor into the ascending row of seen ids, the entries ahead of
//                   it in a register across the tile's product, a 64-bit mask that clears a candidate before it is compared
//   k_rank_metrics  the lists against a held-out matrix: hits by binary search, precision / recall / ndcg / hit rate per user;
//   k_rank_metrics_fold  their means over the eligible users, added by ascending user in one chain
//   k_cross_pairs   the scores of the stored entries of a [nU x nV] matrix: a wavefront per 16 entries of a row, their rows of
//                   qV gathered, the user's q_u in all 16 rows of the matrix instruction -- the tile's chain per pair
//   k_cross_rank_among   the K best of every row of such a matrix: one wavefront per user over the scores of its entries
//   k_cross_rank_of  the tile over (item chunk, user tile, pass): no list, the items counted against the scores of up to 64
//                   held-out pairs per user, held in registers; k_rank_of_close, k_rank_of_candidates: -1 for a seen item, nV - seen
// The bits of a score depend on its two rows and the model alone: every output of the matrix instruction is its own chain
// over the factors, edge tiles run on zero operands, and a row's scalar is added the same way wherever the row stands.
// No kernel waits for another workgroup, a flag in memory or the host.
#include <algorithm>

#include "cross.h"
#include "dataset_ops.h"
#include "fm_device.h"
#include "plan.h"

namespace nfm {

namespace {

typedef double v4d_t __attribute__((ext_vector_type(4)));

constexpr int kCrossLD = kCrossKS + 2;  // doubles per staged row: 16 rows x 2 factors of a half wave fall into 32 different 8-byte banks
constexpr int kCrossSLD = kCrossTV + 1;  // doubles per row of the tile of scores
constexpr int32_t kNoItem = 2147483647;  // the id of an empty list slot: ranks below every item
static_assert(kBlock == 256 && kCrossTU == 32 && kCrossTV == 64 && kCrossKS % 4 == 0, "the staging and the wave -> subtile map below are written for these");
static_assert(kCrossTU * kCrossSLD <= kCrossTV * kCrossLD, "the tile of scores reuses the staged item rows");

// ---- one side ----
template <int L, int SPLIT>
__global__ __launch_bounds__(kBlock) void k_cross_side(CsrView X, ModelView M, int64_t col0, int n_aug, int is_u, int Kq, double* __restrict__ Q,
                                                       double* __restrict__ A) {
  constexpr int LPS = L * SPLIT, SPW = kWave / LPS;
  const int lane = threadIdx.x & (kWave - 1);
  const int sidx = lane / LPS, slot = (lane / L) % SPLIT, l = lane % L;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const double sw = M.sc[SC_SCALE_W], b = is_u ? M.sc[SC_INTERCEPT] : 0.0;
  const dev::PlainParams ps{M.P, M.sc[SC_SCALE_P]};
  const double* w = M.w + col0;
  const int rstride = (int)M.rs * M.Kp;
  for (int64_t i0 = wave0 * SPW; i0 < X.n; i0 += nwaves * SPW) {
    const int64_t i = i0 + sidx;
    const bool valid = i < X.n;
    const int64_t q0 = valid ? X.indptr[i] : 0;
    const int m = valid ? (int)(X.indptr[i + 1] - q0) : 0;
    const int m_tot = valid ? m + n_aug : 0;  // (the dummy feature: X.d is the model's d on the U side)
    double part = 0.0;
    for (int q = slot * L + l; q < m; q += LPS) part += (sw * w[X.indices[q0 + q]]) * X.data[q0 + q];
    for (int o = 0; o < M.nb; ++o) {  // one order: the kc blocks of its factors
      const size_t blk = M.row(o, 0) * M.Kp + (size_t)col0 * rstride;  // row j of this side is row col0 + j of the model
      double2 A1, A2;
      dev::anova_fwd_deg2<L, SPLIT>(ps, X, q0, m, m_tot, blk, rstride, slot, l, A1, A2);
      const double* lm = M.lams + (size_t)(o % M.kc) * M.Kp;
      const double lam0 = lm[2 * l], lam1 = lm[2 * l + 1];
      if (slot == 0) {  // every slot holds the same totals
        const double kx = (A1.x * A1.x - A2.x) / 2.0, ky = (A1.y * A1.y - A2.y) / 2.0;
        part += kx * lam0 + ky * lam1;
        if (valid) {
          double2 qv = A1;
          if (is_u) {
            qv.x = lam0 * A1.x;
            qv.y = lam1 * A1.y;
          }
          *reinterpret_cast<double2*>(Q + (size_t)i * Kq + (size_t)o * M.Kp + 2 * l) = qv;
        }
      }
    }
#pragma unroll
    for (int s = 1; s < LPS; s <<= 1) part += dev::shfl_xor_d(part, s);
    if (valid && slot == 0 && l == 0) A[i] = b + part;
  }
}

template <int L, int SPLIT>
static int launch_side(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int64_t col0, int n_aug, int is_u, int Kq, double* Q, double* A) {
  constexpr int SPW = kWave / (L * SPLIT);
  int64_t blocks = (X.n + (int64_t)kWavesPerBlock * SPW - 1) / ((int64_t)kWavesPerBlock * SPW);
  const int64_t cap = (int64_t)ctx->n_cu * 32;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL((k_cross_side<L, SPLIT>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, X, M, col0, n_aug, is_u, Kq, Q, A);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// The row slots of a sample set the order in which its entries are summed (fm_device.h), so they are a function of the model's
// lanes per row alone: not of the set's size or mean row length (choose_split looks at both) and of no environment variable.  A
// row's q, a and c then have the same bits whatever set the row stands in.  Four slots where the wavefront has them: the chain
// of a long row is a quarter as long, and the launch (0.1 ms for 1e5 rows) is nowhere near the product's time.
template <int L>
static int launch_side_L(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int64_t col0, int n_aug, int is_u, int Kq, double* Q, double* A) {
  constexpr int R = kWave / L, SPLIT = R >= 4 ? 4 : R;
  return launch_side<L, SPLIT>(ctx, X, M, col0, n_aug, is_u, Kq, Q, A);
}

// what one wavefront has written to LDS is what its lanes read next
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- one side of a field-aware model (cross.h: the factorisation) ----
// A team of T lanes owns a row; a workgroup holds blockDim.x / T teams, each with Kq doubles of LDS: the row's accumulators,
// indexed by a field that is read from memory.  The parameters are feature-major, so what an entry (j, f, x) adds is ONE
// contiguous run of RL = Fo * Kp doubles (Fo: the other side's field count): the user side reads the rows FU .. F - 1 of
// feature j and adds them to acc[f][0 .. FV)[:], as contiguous as the run; the item side reads the rows 0 .. FU - 1 of feature
// dU + j and adds row f' to acc[f'][g][:], a scatter with stride FV * Kp.  Lane t of the team owns the 16-byte words
// t, t + T, ... of the run and with them a fixed set of accumulators, which no other lane touches: every accumulator is one
// chain over the row's entries in storage order, x * (scale * p) added by fma, whatever T is and wherever the row stands.
// The run is walked in chunks of kFfmChunk words per lane; the next chunk -- of this entry or the first of the next one -- is
// in flight while this one is added.  The row's own scalar is k_ffm_predict's ordered-pair walk over the row's own entries,
// the pairs dealt to the team's T / L slots, with the side's column and field offsets; its order is a function of T, and T
// of the model and the two field counts alone (ffm_side_team).
constexpr int kFfmChunk = 4;
constexpr int kFfmMaxKq = 4096;            // 32 KiB of accumulators per row
constexpr size_t kFfmLdsBudget = 128 << 10;  // per workgroup, of the CU's 160 KiB

struct FfmSide {
  int64_t col0;  // the side's first column in the model
  int F;         // the model's fields
  int f0;        // the side's first field: what is added to a stored field in the row's own pairs
  int Fs, Fo;    // the side's field count, the other side's
  int o0;        // the first of the other side's fields: where an entry's run starts
  int FV;        // the item side's field count (the layout's inner field)
  int lgL;       // Kp == 2 << lgL
  int Kq;
};

struct FfmChunk {
  double2 v[kFfmChunk];
  double x;
  int f;
};

template <int T>
__device__ __forceinline__ void ffm_chunk_load(FfmChunk& c, const dev::PlainParams& ps, const CsrView& X, const FfmSide& S, int Kp, int64_t q0, int m, int nch,
                                               int it, int t) {
  const int q = it / nch, ch = it - q * nch;
  c.x = 0.0;
  c.f = 0;
#pragma unroll
  for (int i = 0; i < kFfmChunk; ++i) c.v[i] = double2{0.0, 0.0};
  if (q >= m) return;
  const int j = X.indices[q0 + q];
  c.x = X.data[q0 + q];
  c.f = X.fields[q0 + q];
  const size_t base = ((size_t)(S.col0 + j) * S.F + S.o0) * Kp;
  const int rl2 = S.Fo << S.lgL;  // the run in 16-byte words
#pragma unroll
  for (int i = 0; i < kFfmChunk; ++i) {
    const int r2 = (ch * kFfmChunk + i) * T + t;
    if (r2 < rl2) c.v[i] = ps.load(base + 2 * (size_t)r2);
  }
}

template <int T, bool ITEM>
__device__ __forceinline__ void ffm_chunk_add(const FfmChunk& c, const FfmSide& S, double* acc, int nch, int it, int t) {
  if ((unsigned)c.f >= (unsigned)S.Fs) return;  // (a field the side does not have: nothing to add it to)
  const int ch = it % nch, rl2 = S.Fo << S.lgL;
#pragma unroll
  for (int i = 0; i < kFfmChunk; ++i) {
    const int r2 = (ch * kFfmChunk + i) * T + t;
    if (r2 < rl2) {
      // user: acc[f][g][s] with (g, s) = the run's offset; item: acc[f'][f][s] with (f', s) = the run's offset
      const int a2 = ITEM ? ((((r2 >> S.lgL) * S.FV + c.f) << S.lgL) + (r2 & ((1 << S.lgL) - 1))) : c.f * rl2 + r2;
      double2 a = *reinterpret_cast<double2*>(acc + 2 * a2);
      a.x = fma(c.x, c.v[i].x, a.x);
      a.y = fma(c.x, c.v[i].y, a.y);
      *reinterpret_cast<double2*>(acc + 2 * a2) = a;
    }
  }
}

// Q [X.n][Kq], A [X.n].  The workgroup's rows: blockDim.x / T, each with Kq doubles of dynamic LDS.
template <int T, bool ITEM>
__global__ __launch_bounds__(kBlock) void k_cross_side_ffm(CsrView X, ModelView M, FfmSide S, double* __restrict__ Q, double* __restrict__ A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cross_dyn[];
  const int t = threadIdx.x % T, team = threadIdx.x / T, teams = blockDim.x / T;
  double* acc = reinterpret_cast<double*>(cross_dyn) + (size_t)team * S.Kq;
  const int Kp = M.Kp, L = 1 << S.lgL, R = T / L, slot = t >> S.lgL, l = t & (L - 1);
  const int rl2 = S.Fo << S.lgL, nch = (rl2 + T * kFfmChunk - 1) / (T * kFfmChunk);
  const double sw = M.sc[SC_SCALE_W], b = ITEM ? 0.0 : M.sc[SC_INTERCEPT];
  const dev::PlainParams ps{M.P, M.sc[SC_SCALE_P]};
  const double* w = M.w + S.col0;
  for (int64_t i0 = (int64_t)blockIdx.x * teams; i0 < X.n; i0 += (int64_t)gridDim.x * teams) {  // the same trips for every lane
    const int64_t i = i0 + team;
    const bool valid = i < X.n;
    const int64_t q0 = valid ? X.indptr[i] : 0;
    const int m = valid ? (int)(X.indptr[i + 1] - q0) : 0;
    for (int p = t; 2 * p < S.Kq; p += T) *reinterpret_cast<double2*>(acc + 2 * p) = double2{0.0, 0.0};  // every row, the padding too
    wave_lds_fence();  // (a team is part of one wavefront) the clearing lane is not the owning one
    const int nit = m * nch;
    FfmChunk cur, nxt;
    ffm_chunk_load<T>(cur, ps, X, S, Kp, q0, m, nch, 0, t);
    for (int it = 0; it < nit; ++it) {
      ffm_chunk_load<T>(nxt, ps, X, S, Kp, q0, m, nch, it + 1, t);
      ffm_chunk_add<T, ITEM>(cur, S, acc, nch, it, t);
      cur = nxt;
    }
    // the row's own scalar
    double part = 0.0;
    for (int q = t; q < m; q += T) part += (sw * w[X.indices[q0 + q]]) * X.data[q0 + q];
    const int64_t npairs = (int64_t)m * m;
    for (int64_t pb = 0; pb < npairs; pb += R) {
      const int64_t pr = pb + slot;
      if (pr < npairs) {
        const int a = (int)(pr / m), c2 = (int)(pr % m);
        const int j1 = X.indices[q0 + a], j2 = X.indices[q0 + c2];
        const int g1 = X.fields[q0 + a], g2 = X.fields[q0 + c2];
        if (j1 < j2 && (unsigned)g1 < (unsigned)S.Fs && (unsigned)g2 < (unsigned)S.Fs) {
          const int f1 = S.f0 + g1, f2 = S.f0 + g2;
          const double2 u = ps.load(M.row(f2, S.col0 + j1) * Kp + 2 * l);
          const double2 v = ps.load(M.row(f1, S.col0 + j2) * Kp + 2 * l);
          part += (X.data[q0 + a] * X.data[q0 + c2]) * (u.x * v.x + u.y * v.y);
        }
      }
    }
#pragma unroll
    for (int s = 1; s < T; s <<= 1) part += dev::shfl_xor_d(part, s);
    wave_lds_fence();  // the owners' sums are what any lane of the team writes out
    if (valid) {
      for (int p = t; 2 * p < S.Kq; p += T) *reinterpret_cast<double2*>(Q + (size_t)i * S.Kq + 2 * p) = *reinterpret_cast<const double2*>(acc + 2 * p);
      if (t == 0) A[i] = b + part;
    }
    wave_lds_fence();  // written out before the next row's clear
  }
}

// lanes per row: the run's 16-byte words, between the model's lanes per parameter row (at least 16: the pair walk of a long
// row wants slots) and a wavefront
static int ffm_side_team(int Fo, int L) {
  int T = 16;
  while (T < kWave && T < Fo * L) T <<= 1;
  return T;
}

template <int T, bool ITEM>
static int launch_side_ffm(nfm_ctx* ctx, const CsrView& X, const ModelView& M, const FfmSide& S, double* Q, double* A) {
  int teams = kBlock / T;
  while (teams > 1 && (size_t)teams * S.Kq * sizeof(double) > kFfmLdsBudget) teams >>= 1;  // (Kq <= kFfmMaxKq: four rows always fit)
  const size_t lds = (size_t)teams * S.Kq * sizeof(double);
  const void* kernel = reinterpret_cast<const void*>(k_cross_side_ffm<T, ITEM>);
  if (lds > 65536) NFM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // eight workgroups a CU are all its wavefront slots; more rows are walked with that stride
  const int64_t blocks = std::min<int64_t>((X.n + teams - 1) / teams, (int64_t)ctx->n_cu * 8);
  hipLaunchKernelGGL((k_cross_side_ffm<T, ITEM>), dim3((unsigned)blocks), dim3(teams * T), lds, ctx->stream, X, M, S, Q, A);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

template <bool ITEM>
static int launch_side_ffm_T(nfm_ctx* ctx, const CsrView& X, const ModelView& M, const FfmSide& S, double* Q, double* A) {
  switch (ffm_side_team(S.Fo, M.L)) {
    case 16: return launch_side_ffm<16, ITEM>(ctx, X, M, S, Q, A);
    case 32: return launch_side_ffm<32, ITEM>(ctx, X, M, S, Q, A);
    default: return launch_side_ffm<64, ITEM>(ctx, X, M, S, Q, A);
  }
}

// ---- the tile ----
// One step of kCrossKS factors of a tile's operands on their way from global memory to LDS, in registers: the loads of the next
// step (or of the next tile's first step) are in flight while the matrix instructions of this one run.
struct CrossStage {
  double2 a[2];  // users: row t / 8, four factors from 4 (t % 8)
  double2 b[4];  // items: row t / 4, eight factors from 8 (t % 4)
};
__device__ __forceinline__ void stage_load(CrossStage& g, const double* __restrict__ qU, const double* __restrict__ qV, int Kq, int64_t u0, int64_t nU,
                                           int64_t v0, int64_t nV, int s0) {
  const int t = threadIdx.x;
  const int ks = Kq - s0 < kCrossKS ? Kq - s0 : kCrossKS;  // a multiple of 4
  {
    const int r = t >> 3, c = 4 * (t & 7);
    g.a[0] = g.a[1] = double2{0.0, 0.0};  // rows past nU (and factors past Kq) are zero operands
    if (u0 + r < nU && c < ks) {
      const double* p = qU + (size_t)(u0 + r) * Kq + s0 + c;
      g.a[0] = *reinterpret_cast<const double2*>(p);
      g.a[1] = *reinterpret_cast<const double2*>(p + 2);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = t >> 2, c = 8 * (t & 3) + 4 * h;
    g.b[2 * h] = g.b[2 * h + 1] = double2{0.0, 0.0};
    if (v0 + r < nV && c < ks) {
      const double* p = qV + (size_t)(v0 + r) * Kq + s0 + c;
      g.b[2 * h] = *reinterpret_cast<const double2*>(p);
      g.b[2 * h + 1] = *reinterpret_cast<const double2*>(p + 2);
    }
  }
}
__device__ __forceinline__ void stage_store(const CrossStage& g, double* As, double* Bs) {
  const int t = threadIdx.x;
  *reinterpret_cast<double2*>(As + (t >> 3) * kCrossLD + 4 * (t & 7)) = g.a[0];
  *reinterpret_cast<double2*>(As + (t >> 3) * kCrossLD + 4 * (t & 7) + 2) = g.a[1];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    *reinterpret_cast<double2*>(Bs + (t >> 2) * kCrossLD + 8 * (t & 3) + 4 * h) = g.b[2 * h];
    *reinterpret_cast<double2*>(Bs + (t >> 2) * kCrossLD + 8 * (t & 3) + 4 * h + 2) = g.b[2 * h + 1];
  }
}

// acc[h][r] of lane l of wave w: user row 16 h + (l >> 4) + 4 r, item column 16 w + (l & 15) of the tile at (u0, v0) -- the
// C/D map of v_mfma_f64_16x16x4_f64 (not the f32 one); A and B operands: one double per lane, row / column l & 15, factor
// l >> 4 of the four.  As, Bs: kCrossTU and kCrossTV staged rows of kCrossLD doubles.  g holds the tile's first step on entry
// (stage_load at s0 = 0) and, on return, the first step of the tile at v_next (v_next < 0: nothing).  Every lane of the
// workgroup calls it; on return the lanes may still be reading As / Bs (the caller syncs before reuse).
__device__ __forceinline__ void cross_tile(const double* __restrict__ qU, const double* __restrict__ qV, int Kq, int64_t u0, int64_t nU, int64_t v0,
                                           int64_t nV, int64_t v_next, double* As, double* Bs, CrossStage& g, v4d_t (&acc)[2]) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  acc[0] = v4d_t{0.0, 0.0, 0.0, 0.0};
  acc[1] = v4d_t{0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < Kq; s0 += kCrossKS) {
    const int ks = Kq - s0 < kCrossKS ? Kq - s0 : kCrossKS;
    __syncthreads();  // the last step's operands (and a caller's tile of scores) have been read
    stage_store(g, As, Bs);
    __syncthreads();
    if (s0 + kCrossKS < Kq)
      stage_load(g, qU, qV, Kq, u0, nU, v0, nV, s0 + kCrossKS);
    else if (v_next >= 0)
      stage_load(g, qU, qV, Kq, u0, nU, v_next, nV, 0);
    const int r = lane & 15, f = lane >> 4;
    for (int k4 = 0; k4 < ks; k4 += 4) {
      const double a0 = As[r * kCrossLD + k4 + f], a1 = As[(16 + r) * kCrossLD + k4 + f], bb = Bs[(16 * wv + r) * kCrossLD + k4 + f];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bb, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bb, acc[1], 0, 0, 0);
    }
  }
}

// a row's two scalars and the product, always in this order
__device__ __forceinline__ double cross_score(double a_u, double c_v, double dot) { return (a_u + c_v) + dot; }

__global__ __launch_bounds__(kBlock) void k_cross_scores(const double* __restrict__ qU, const double* __restrict__ qV, const double* __restrict__ aU,
                                                         const double* __restrict__ cV, int Kq, int64_t u_begin, int64_t u_end, int64_t nV,
                                                         double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double As[kCrossTU * kCrossLD];
  __shared__ __attribute__((aligned(16))) double Bs[kCrossTV * kCrossLD];
  const int64_t u0 = u_begin + (int64_t)blockIdx.y * kCrossTU, v0 = (int64_t)blockIdx.x * kCrossTV;
  v4d_t acc[2];
  CrossStage g;
  stage_load(g, qU, qV, Kq, u0, u_end, v0, nV, 0);
  cross_tile(qU, qV, Kq, u0, u_end, v0, nV, -1, As, Bs, g, acc);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int64_t col = v0 + 16 * wv + (lane & 15);
  if (col >= nV) return;
  const double c = cV[col];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = u0 + 16 * h + (lane >> 4) + 4 * r;
      if (row < u_end) out[(size_t)(row - u_begin) * nV + col] = cross_score(aU[row], c, acc[h][r]);
    }
}

// ---- ranking ----
// (score, id) ranks before (score', id') if score > score', or they are equal and id < id'; NaN below every number, NaN
// against NaN by id.  key(): the bits of a double as an unsigned integer that ascends with the number; -0 == +0; NaN -> 0.
__host__ __device__ __forceinline__ uint64_t rank_key(uint64_t bits) {
  if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return 0;
  if ((bits << 1) == 0) return 0x8000000000000000ull;
  return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}
__host__ __device__ __forceinline__ bool ranks_before(uint64_t key_a, int32_t id_a, uint64_t key_b, int32_t id_b) {
  return key_a > key_b || (key_a == key_b && id_a < id_b);
}

// The list of one user: K (bits, id) in LDS, best first, empty slots (NaN, kNoItem) last.  One wavefront puts a candidate
// that ranks before the last entry in its place: every lane counts the entries of its slots that rank before the candidate,
// the entries from there on move down one slot, the last one leaves.
__device__ __forceinline__ void list_insert(uint64_t* lb, int32_t* li, int K, uint64_t cbits, int32_t cid, int lane) {
  const uint64_t ckey = rank_key(cbits);
  uint64_t eb[kCrossMaxTopK / kWave];
  int32_t ei[kCrossMaxTopK / kWave];
  const int rounds = (K + kWave - 1) / kWave;  // the same for every lane
  int pos = 0;
#pragma unroll
  for (int c = 0; c < kCrossMaxTopK / kWave; ++c) {
    eb[c] = 0;
    ei[c] = kNoItem;
    if (c < rounds) {
      const int p = lane + c * kWave;
      bool before = false;
      if (p < K) {
        eb[c] = lb[p];
        ei[c] = li[p];
        before = ranks_before(rank_key(eb[c]), ei[c], ckey, cid);
      }
      pos += __popcll(__ballot(before));
    }
  }
  wave_lds_fence();
#pragma unroll
  for (int c = 0; c < kCrossMaxTopK / kWave; ++c) {
    const int p = lane + c * kWave;
    if (c < rounds && p >= pos && p + 1 < K) {
      lb[p + 1] = eb[c];
      li[p + 1] = ei[c];
    }
  }
  if (lane == 0 && pos < K) {
    lb[pos] = cbits;
    li[pos] = cid;
  }
  wave_lds_fence();
}

// The seen ids of one window as a mask, bit b = item v0 + b: the lanes named by `in` hold ids of [v0, v0 + kCrossTV).
__device__ __forceinline__ unsigned long long seen_bits(int32_t id, unsigned long long in, int64_t v0) {
  unsigned long long bits = 0;
  while (in) {
    const int src = __ffsll(in) - 1;
    in &= in - 1;
    bits |= 1ull << (__shfl(id, src, kWave) - (int32_t)v0);
  }
  return bits;
}

constexpr int kSeenAhead = kWave / (kCrossTU / kWavesPerBlock);  // ids of a user's row that its wave holds ahead of the cursor
constexpr int32_t kNoSeen = 2147483647;  // past every window: a lane with nothing ahead
constexpr size_t kSeenLds = sizeof(int64_t) * 2 * kCrossTU;  // the cursors: (next, end) per user

// what the lanes of wave wv hold ahead: lane l the entry (l % kSeenAhead) past the cursor of user wv * 8 + l / kSeenAhead
__device__ __forceinline__ int32_t seen_ahead(const int32_t* __restrict__ sidx, const int64_t* curs, int wv, int lane) {
  const int rl = wv * (kCrossTU / kWavesPerBlock) + lane / kSeenAhead;
  const int64_t at = curs[2 * rl] + lane % kSeenAhead;
  return at < curs[2 * rl + 1] ? sidx[at] : kNoSeen;
}

// grid: x = item chunk, y = user tile.  pbits / pids [nU][chunks][K].
// SEEN: sptr [nU + 1], sidx: per user the ids that are no candidates, ascending inside the row (repeats allowed).  The wave
// that ranks a user owns that user's cursor: the next entry of the row not below the tile, and the first one not below the
// chunk's end, as positions in sidx (int64: no bound on a row or on the matrix), in LDS.  It holds the kSeenAhead entries
// past each of its eight cursors in one register, loaded before the tile's product and read after it; a window that takes
// all of them (a dense stretch, repeats) goes on in rounds of a wavefront's width straight from memory.
template <bool SEEN>
__global__ __launch_bounds__(kBlock) void k_cross_topk(const double* __restrict__ qU, const double* __restrict__ qV, const double* __restrict__ aU,
                                                       const double* __restrict__ cV, int Kq, int64_t nU, int64_t nV, int64_t chunk_len, int K,
                                                       uint64_t* __restrict__ pbits, int32_t* __restrict__ pids, const int64_t* __restrict__ sptr,
                                                       const int32_t* __restrict__ sidx) {
  __shared__ __attribute__((aligned(16))) double As[kCrossTU * kCrossLD];
  __shared__ __attribute__((aligned(16))) double Bs[kCrossTV * kCrossLD];
  extern __shared__ __attribute__((aligned(16))) unsigned char cross_dyn[];
  int64_t* curs = reinterpret_cast<int64_t*>(cross_dyn);                                      // SEEN: [kCrossTU][2]
  uint64_t* lbits = reinterpret_cast<uint64_t*>(cross_dyn + (SEEN ? kSeenLds : 0));           // [kCrossTU][K]
  int32_t* lids = reinterpret_cast<int32_t*>(lbits + (size_t)kCrossTU * K);  // [kCrossTU][K]
  double* Sc = Bs;  // the tile of scores, [kCrossTU][kCrossSLD], once the item rows have been used
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const int64_t u0 = (int64_t)blockIdx.y * kCrossTU;
  const int64_t v_begin = (int64_t)blockIdx.x * chunk_len, v_end = v_begin + chunk_len < nV ? v_begin + chunk_len : nV;
  for (int p = t; p < kCrossTU * K; p += kBlock) {
    lbits[p] = 0x7ff8000000000000ull;
    lids[p] = kNoItem;
  }
  int32_t ahead = kNoSeen;
  if constexpr (SEEN) {
    // lanes 0 and 1 of a user's kSeenAhead: the first entry of the row not below v_begin, and not below v_end
    const int rl = wv * (kCrossTU / kWavesPerBlock) + lane / kSeenAhead, e = lane % kSeenAhead;
    if (e < 2) {
      int64_t lo = 0, hi = 0;
      if (u0 + rl < nU) {
        lo = sptr[u0 + rl];
        hi = sptr[u0 + rl + 1];
      }
      const int64_t want = e ? v_end : v_begin;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sidx[mid] < want) lo = mid + 1; else hi = mid;
      }
      curs[2 * rl + e] = lo;
    }
    wave_lds_fence();
    ahead = seen_ahead(sidx, curs, wv, lane);
  }
  CrossStage g;
  stage_load(g, qU, qV, Kq, u0, nU, v_begin, nV, 0);
  for (int64_t v0 = v_begin; v0 < v_end; v0 += kCrossTV) {
    v4d_t acc[2];
    cross_tile(qU, qV, Kq, u0, nU, v0, nV, v0 + kCrossTV < v_end ? v0 + kCrossTV : -1, As, Bs, g, acc);
    __syncthreads();  // the item rows have been read: their place takes the scores
    {
      const int cl = 16 * wv + (lane & 15);
      const int64_t col = v0 + cl;
      const double c = col < nV ? cV[col] : 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = 16 * h + (lane >> 4) + 4 * r;
          const double a = u0 + rl < nU ? aU[u0 + rl] : 0.0;
          Sc[rl * kCrossSLD + cl] = cross_score(a, c, acc[h][r]);
        }
    }
    __syncthreads();
    // wave w ranks the users 8 w .. 8 w + 7 of the tile, one item per lane
    // SEEN: the lanes whose entry ahead falls into this tile's window; nearly always none
    const unsigned long long in_all = SEEN ? __ballot((int64_t)ahead < v0 + kCrossTV) : 0ull;
    for (int ru = 0; ru < kCrossTU / kWavesPerBlock; ++ru) {
      const int rl = wv * (kCrossTU / kWavesPerBlock) + ru;
      if (u0 + rl >= nU) break;
      uint64_t* lb = lbits + (size_t)rl * K;
      int32_t* li = lids + (size_t)rl * K;
      const int64_t j = v0 + lane;
      const uint64_t bits = (uint64_t)__double_as_longlong(Sc[rl * kCrossSLD + lane]);
      const uint64_t key = rank_key(bits);
      bool pass = j < v_end && ranks_before(key, (int32_t)j, rank_key(lb[K - 1]), li[K - 1]);
      if constexpr (SEEN) {
        const unsigned long long in = in_all & (((1ull << kSeenAhead) - 1) << (ru * kSeenAhead));
        if (in) {  // the same for every lane
          unsigned long long seen = seen_bits(ahead, in, v0);
          int64_t pos = curs[2 * rl] + __popcll(in);
          if (__popcll(in) == kSeenAhead) {  // the window may go on: rounds of kWave ids until one ends inside the round
            const int64_t end = curs[2 * rl + 1];
            for (;;) {
              const int32_t id = pos + lane < end ? sidx[pos + lane] : kNoSeen;
              const unsigned long long more = __ballot((int64_t)id < v0 + kCrossTV);
              seen |= seen_bits(id, more, v0);
              pos += __popcll(more);
              if (__popcll(more) < kWave) break;
            }
          }
          wave_lds_fence();  // every lane has read the cursor
          if (lane == 0) curs[2 * rl] = pos;
          pass = pass && !((seen >> lane) & 1);  // before the ballot: a seen item is never compared again, inserted, or evicts
        }
      }
      unsigned long long mask = __ballot(pass);
      while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const uint64_t cbits = (uint64_t)__shfl((long long)bits, src, kWave);
        const int32_t cid = (int32_t)(v0 + src);
        if (ranks_before(rank_key(cbits), cid, rank_key(lb[K - 1]), li[K - 1])) list_insert(lb, li, K, cbits, cid, lane);
      }
    }
    if constexpr (SEEN) {
      if (in_all && v0 + kCrossTV < v_end) {  // a cursor moved: the entries ahead of the next tile, in flight across its product
        wave_lds_fence();
        ahead = seen_ahead(sidx, curs, wv, lane);
      }
    }
    // (cross_tile opens with a barrier: the scores have been read before the next tile's rows are staged)
  }
  __syncthreads();
  for (int p = t; p < kCrossTU * K; p += kBlock) {
    const int rl = p / K, e = p % K;
    if (u0 + rl < nU) {
      const size_t at = ((size_t)(u0 + rl) * gridDim.x + blockIdx.x) * K + e;
      pbits[at] = lbits[p];
      pids[at] = lids[p];
    }
  }
}

// One lane per entry of the chunks' lists: its rank among all of a user's entries is its place in its own (sorted) list
// plus, for every other list, the entries there that rank before it (a binary search: the lists are sorted).  The ranks are
// distinct -- no two entries of a user share an id -- so the entries of rank < K fill the K places.
__global__ __launch_bounds__(kBlock) void k_cross_merge(const uint64_t* __restrict__ pbits, const int32_t* __restrict__ pids, int64_t nU, int chunks, int K,
                                                        int64_t* __restrict__ ids, double* __restrict__ scores) {
  const int64_t total = nU * chunks * K;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int p = (int)(e % K);
    const int c = (int)((e / K) % chunks);
    const int64_t u = e / K / chunks;
    const int32_t id = pids[e];
    if (id == kNoItem) continue;
    const uint64_t bits = pbits[e], key = rank_key(bits);
    int64_t rank = p;
    for (int c2 = 0; c2 < chunks && rank < K; ++c2) {
      if (c2 == c) continue;
      const size_t base = ((size_t)u * chunks + c2) * K;
      int lo = 0, hi = K;  // the first entry of list c2 that does not rank before this one
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ranks_before(rank_key(pbits[base + mid]), pids[base + mid], key, id)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < K) {
      ids[(size_t)u * K + rank] = id;
      scores[(size_t)u * K + rank] = __longlong_as_double((long long)bits);
    }
  }
}

// the masked path's outputs before the merge: a rank that no candidate fills
__global__ void k_cross_no_item(int64_t n, int64_t* __restrict__ ids, double* __restrict__ scores) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    ids[e] = -1;
    scores[e] = __longlong_as_double(0x7ff8000000000000ll);
  }
}

// ---- ranking metrics ----
// One wavefront per user, one lane per rank: a hit is an id of the list found in the user's held-out row (ascending, distinct:
// a binary search).  per [nU][5]: precision, recall, ndcg, hit rate and 1 of an eligible user (a held-out row that is not
// empty), five zeros of any other.  The DCG adds disc[r] of the hits by ascending r, every lane the same chain.
__global__ __launch_bounds__(kBlock) void k_rank_metrics(int64_t nU, int K, const int64_t* __restrict__ ids, const int64_t* __restrict__ tptr,
                                                         const int32_t* __restrict__ tidx, const double* __restrict__ disc,
                                                         const double* __restrict__ idisc, double* __restrict__ per) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nU; u += nwaves) {
    const int64_t t0 = tptr[u], t1 = tptr[u + 1];
    int hits = 0;
    double dcg = 0.0;
    for (int r0 = 0; r0 < K && t1 > t0; r0 += kWave) {
      const int r = r0 + lane;
      const int64_t id = r < K ? ids[(size_t)u * K + r] : -1;
      bool hit = false;
      if (id >= 0) {
        int64_t lo = t0, hi = t1;
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (tidx[mid] < id) lo = mid + 1; else hi = mid;
        }
        hit = lo < t1 && tidx[lo] == id;
      }
      unsigned long long m = __ballot(hit);
      hits += __popcll(m);
      while (m) {
        dcg += disc[r0 + __ffsll(m) - 1];
        m &= m - 1;
      }
    }
    if (lane < 5) {
      double v = 0.0;
      if (t1 > t0) {
        const int64_t len = t1 - t0;
        v = lane == 0 ? (double)hits / (double)K
          : lane == 1 ? (double)hits / (double)len
          : lane == 2 ? dcg / idisc[(len < K ? len : K) - 1]
          : lane == 3 ? (hits > 0 ? 1.0 : 0.0) : 1.0;
      }
      per[(size_t)u * 5 + lane] = v;
    }
  }
}

// The fold: lane c adds column c of per by ascending user, one chain -- the same bits from run to run.  out[0..3]: the sums
// over the count, out[4]: the count (0 / 0 = NaN where no user is eligible).
__global__ void k_rank_metrics_fold(int64_t nU, const double* __restrict__ per, double* __restrict__ out) {
  __shared__ double tot[5];
  const int c = threadIdx.x;
  if (c < 5) {
    double acc = 0.0;
#pragma unroll 8
    for (int64_t u = 0; u < nU; ++u) acc += per[(size_t)u * 5 + c];
    tot[c] = acc;
  }
  __syncthreads();
  if (c < 5) out[c] = c < 4 ? tot[c] / tot[4] : tot[4];
}

// ---- given pairs ----
// The scores of stored entries of a [nU x nV] matrix instead of every pair: per entry a gathered row of qV, the same chain.
// A block is up to kCrossPB consecutive entries of one user's row; the blocks of all rows form one list (blk: the exclusive
// scan of the rows' block counts), so one long row and many short ones spread over the chip alike.  A wavefront takes a
// block: the 16 items are the 16 columns of v_mfma_f64_16x16x4_f64 and the user's q_u is the A operand in all 16 rows, so
// every row of the result is cross_tile's chain for (u, item) -- accumulator from 0, the factors ascending four at a time,
// zero operands past the block's end -- and row 0 (register 0 of lanes 0 .. 15) is written.  15 of 16 rows of the matrix unit
// are spent on purpose: the block is 16 gathered rows of Kq doubles, and those, not the instruction, set its time.
constexpr int kCrossPB = 16;
static_assert(kCrossPB * 4 == kWave && kCrossKS == 32, "four lanes load one item's step of 32 factors, eight each");

struct PairBlock {
  int64_t u = 0, e0 = 0;  // the user, the block's first entry
  int cnt = 0;            // its entries (0: past the list)
  int32_t j = 0;          // lane l < cnt: the item of entry e0 + l
};
__device__ __forceinline__ PairBlock pair_block(int64_t b, int64_t nB, int64_t nU, const int64_t* __restrict__ blk, const int64_t* __restrict__ indptr,
                                                const int32_t* __restrict__ idx, int lane) {
  PairBlock B;
  if (b >= nB) return B;
  int64_t lo = 0, hi = nU - 1;  // the last row whose first block is not past b: blk[nU] = nB > b, so that row owns b
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  B.u = lo;
  B.e0 = indptr[lo] + (b - blk[lo]) * kCrossPB;
  const int64_t left = indptr[lo + 1] - B.e0;
  B.cnt = left < kCrossPB ? (int)left : kCrossPB;
  if (lane < B.cnt) B.j = idx[B.e0 + lane];
  return B;
}

// One step of kCrossKS factors of a block on its way to the matrix instruction, in registers.  b: item row lane / 4, eight
// factors from 8 (lane % 4), as contiguous 16-byte words (stage_load's item half); a: the user's factors already where
// the A operand wants them, factor 4 i + lane / 16 of the step -- 16 lanes read one address, so no LDS is needed for q_u
// and the registers do not grow with Kq.
struct PairStage {
  double2 b[4];
  double a[kCrossKS / 4];
};
__device__ __forceinline__ void pair_load(PairStage& g, const double* __restrict__ qU, const double* __restrict__ qV, int Kq, const PairBlock& B, int s0,
                                          int lane) {
  const int ks = Kq - s0 < kCrossKS ? Kq - s0 : kCrossKS;  // a multiple of 4
  const int r = lane >> 2, f = lane >> 4;
  const int32_t j = __shfl(B.j, r, kWave);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 8 * (lane & 3) + 4 * h;
    g.b[2 * h] = g.b[2 * h + 1] = double2{0.0, 0.0};  // entries past the block's end (and factors past Kq) are zero operands
    if (r < B.cnt && c < ks) {
      const double* p = qV + (size_t)j * Kq + s0 + c;
      g.b[2 * h] = *reinterpret_cast<const double2*>(p);
      g.b[2 * h + 1] = *reinterpret_cast<const double2*>(p + 2);
    }
  }
#pragma unroll
  for (int i = 0; i < kCrossKS / 4; ++i) g.a[i] = B.cnt > 0 && 4 * i < ks ? qU[(size_t)B.u * Kq + s0 + 4 * i + f] : 0.0;
}

// out[e]: the score of stored entry e.  Nothing here is shared between wavefronts: each has its own kCrossPB staged rows
// (cross_tile's pitch) and orders its own stores and loads.  The loads of the next step -- after the last one, of the next
// block's first step, whose row was found while this block ran -- are in flight across the matrix instructions.
__global__ __launch_bounds__(kBlock) void k_cross_pairs(const double* __restrict__ qU, const double* __restrict__ qV, const double* __restrict__ aU,
                                                        const double* __restrict__ cV, int Kq, int64_t nU, int64_t nB, const int64_t* __restrict__ blk,
                                                        const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double Bs_all[kWavesPerBlock][kCrossPB * kCrossLD];
  const int lane = threadIdx.x & (kWave - 1), f = lane >> 4;
  double* Bs = Bs_all[threadIdx.x >> 6];
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  PairBlock cur = pair_block(b, nB, nU, blk, indptr, idx, lane);
  PairStage g;
  pair_load(g, qU, qV, Kq, cur, 0, lane);
  for (; b < nB; b += stride) {
    const PairBlock nxt = pair_block(b + stride, nB, nU, blk, indptr, idx, lane);
    v4d_t acc = v4d_t{0.0, 0.0, 0.0, 0.0};
    for (int s0 = 0; s0 < Kq; s0 += kCrossKS) {
      const int ks = Kq - s0 < kCrossKS ? Kq - s0 : kCrossKS;
      wave_lds_fence();  // the last step's operands have been read
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<double2*>(Bs + (lane >> 2) * kCrossLD + 8 * (lane & 3) + 4 * h) = g.b[2 * h];
        *reinterpret_cast<double2*>(Bs + (lane >> 2) * kCrossLD + 8 * (lane & 3) + 4 * h + 2) = g.b[2 * h + 1];
      }
      double a[kCrossKS / 4];
#pragma unroll
      for (int i = 0; i < kCrossKS / 4; ++i) a[i] = g.a[i];
      wave_lds_fence();
      if (s0 + kCrossKS < Kq)
        pair_load(g, qU, qV, Kq, cur, s0 + kCrossKS, lane);
      else
        pair_load(g, qU, qV, Kq, nxt, 0, lane);
#pragma unroll
      for (int i = 0; i < kCrossKS / 4; ++i)
        if (4 * i < ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], Bs[(lane & 15) * kCrossLD + 4 * i + f], acc, 0, 0, 0);
    }
    if (lane < cur.cnt) out[cur.e0 + lane] = cross_score(aU[cur.u], cV[cur.j], acc[0]);
    cur = nxt;
  }
}

// cnt[i]: the blocks of row i; cnt[nU] = 0, so that the scan's last entry is their number
__global__ void k_pair_block_counts(int64_t nU, const int64_t* __restrict__ indptr, int64_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nU; i += (int64_t)gridDim.x * blockDim.x)
    cnt[i] = i < nU ? (indptr[i + 1] - indptr[i] + kCrossPB - 1) / kCrossPB : 0;
}

// The K best of the stored entries of every row: idx ascends inside a row (repeats allowed) and sc[e] is the score of entry
// e.  One wavefront per user walks the row kWave entries a round; an entry equal to its predecessor is the same item and is
// skipped.  The list is k_cross_topk's (list_insert), written straight to ids / scores [nU][K]: there are no chunks to
// merge, and a row however long is one wavefront's.
__global__ __launch_bounds__(kBlock) void k_cross_rank_among(int64_t nU, int K, const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                             const double* __restrict__ sc, int64_t* __restrict__ ids, double* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cross_dyn[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  uint64_t* lb = reinterpret_cast<uint64_t*>(cross_dyn) + (size_t)wv * K;                                     // [kWavesPerBlock][K]
  int32_t* li = reinterpret_cast<int32_t*>(reinterpret_cast<uint64_t*>(cross_dyn) + (size_t)kWavesPerBlock * K) + (size_t)wv * K;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + wv; u < nU; u += nwaves) {
    for (int p = lane; p < K; p += kWave) {
      lb[p] = 0x7ff8000000000000ull;
      li[p] = kNoItem;
    }
    wave_lds_fence();
    const int64_t e_begin = indptr[u], e_end = indptr[u + 1];
    for (int64_t e0 = e_begin; e0 < e_end; e0 += kWave) {
      const int64_t e = e0 + lane;
      int32_t id = kNoItem;
      uint64_t bits = 0;
      bool pass = false;
      if (e < e_end) {
        id = idx[e];
        bits = (uint64_t)__double_as_longlong(sc[e]);
        pass = (e == e_begin || idx[e - 1] != id) && ranks_before(rank_key(bits), id, rank_key(lb[K - 1]), li[K - 1]);
      }
      unsigned long long mask = __ballot(pass);
      while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const uint64_t cbits = (uint64_t)__shfl((long long)bits, src, kWave);
        const int32_t cid = __shfl(id, src, kWave);
        if (ranks_before(rank_key(cbits), cid, rank_key(lb[K - 1]), li[K - 1])) list_insert(lb, li, K, cbits, cid, lane);
      }
    }
    for (int p = lane; p < K; p += kWave) {  // an empty slot is (NaN, kNoItem): a rank that no candidate fills
      const bool filled = li[p] != kNoItem;
      ids[(size_t)u * K + p] = filled ? (int64_t)li[p] : -1;
      scores[(size_t)u * K + p] = __longlong_as_double((long long)(filled ? lb[p] : 0x7ff8000000000000ull));
    }
    wave_lds_fence();  // the list has been read before the next user's is laid out
  }
}

// ---- the rank of given items among all of a user's candidates ----
// No list: the items of a tile are counted against thresholds that are known before the launch (k_cross_pairs' bits of the
// held-out pairs).  Wave w owns the users 8 w .. 8 w + 7 of the tile as in k_cross_topk; per user, lane t holds threshold t of
// this pass (64 entries of the user's held-out row from entry 64 * pass on): its key, its id and the count of the chunk's
// candidates that rank before it -- four registers a user, nothing in LDS, nothing in memory until the chunk ends.
constexpr int kRankUsers = kCrossTU / kWavesPerBlock;  // users per wavefront
static_assert(kCrossTV == kWave, "one lane per item of a tile, one bit per item in the seen mask");

__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int src) {  // src: the same in every lane
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// The seen items of user rl inside the window [v0, v0 + kCrossTV) as a mask, as k_cross_topk<true> finds them: `in` names the
// lanes of `ahead` that hold ids of the window (not 0), a window that takes all kSeenAhead of them goes on in rounds of a
// wavefront's width from memory; the user's cursor moves past what was taken.
__device__ __forceinline__ unsigned long long seen_window(const int32_t* __restrict__ sidx, int64_t* curs, int rl, int32_t ahead, unsigned long long in,
                                                          int64_t v0, int lane) {
  unsigned long long seen = seen_bits(ahead, in, v0);
  int64_t pos = curs[2 * rl] + __popcll(in);
  if (__popcll(in) == kSeenAhead) {
    const int64_t end = curs[2 * rl + 1];
    for (;;) {
      const int32_t id = pos + lane < end ? sidx[pos + lane] : kNoSeen;
      const unsigned long long more = __ballot((int64_t)id < v0 + kCrossTV);
      seen |= seen_bits(id, more, v0);
      pos += __popcll(more);
      if (__popcll(more) < kWave) break;
    }
  }
  wave_lds_fence();  // every lane has read the cursor
  if (lane == 0) curs[2 * rl] = pos;
  return seen;
}

// grid: x = item chunk, y = user tile, z = pass (pass0 + z: the entries 64 (pass0 + z) .. of every held-out row).  tptr [nU + 1],
// tidx, thr: the held-out rows in storage order and the score of every entry; cnt [nnz]: zero before the first launch, on
// return of the last one cnt[e] = the candidates of the whole catalogue that rank before entry e.  A workgroup none of whose
// users has an entry in its pass returns at once.  SEEN: as in k_cross_topk; a user without thresholds gets an empty cursor.
template <bool SEEN>
__global__ __launch_bounds__(kBlock) void k_cross_rank_of(const double* __restrict__ qU, const double* __restrict__ qV, const double* __restrict__ aU,
                                                          const double* __restrict__ cV, int Kq, int64_t nU, int64_t nV, int64_t chunk_len,
                                                          const int64_t* __restrict__ tptr, const int32_t* __restrict__ tidx, const double* __restrict__ thr,
                                                          int64_t pass0, uint32_t* __restrict__ cnt, const int64_t* __restrict__ sptr,
                                                          const int32_t* __restrict__ sidx) {
  __shared__ __attribute__((aligned(16))) double As[kCrossTU * kCrossLD];
  __shared__ __attribute__((aligned(16))) double Bs[kCrossTV * kCrossLD];
  __shared__ int64_t curs[SEEN ? 2 * kCrossTU : 2];  // SEEN: (next, end) per user
  double* Sc = Bs;  // the tile of scores, [kCrossTU][kCrossSLD], once the item rows have been used
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t u0 = (int64_t)blockIdx.y * kCrossTU;
  const int64_t v_begin = (int64_t)blockIdx.x * chunk_len, v_end = v_begin + chunk_len < nV ? v_begin + chunk_len : nV;
  const int64_t first = (pass0 + blockIdx.z) * kWave;  // this pass's first entry, counted from the row's start
  uint64_t tkey[kRankUsers];
  int32_t tid[kRankUsers];
  uint32_t tcnt[kRankUsers];
  int th[kRankUsers];  // the user's thresholds in this pass, 0 .. kWave: the same in every lane
  bool any = false;
#pragma unroll
  for (int ru = 0; ru < kRankUsers; ++ru) {
    const int64_t u = u0 + wv * kRankUsers + ru;
    const int64_t te = u < nU ? tptr[u] + first : 0, left = u < nU ? tptr[u + 1] - te : 0;
    th[ru] = left <= 0 ? 0 : left < kWave ? (int)left : kWave;
    tkey[ru] = 0;
    tid[ru] = kNoItem;
    tcnt[ru] = 0;
    if (lane < th[ru]) {
      tkey[ru] = rank_key((uint64_t)__double_as_longlong(thr[te + lane]));
      tid[ru] = tidx[te + lane];
    }
    any = any || th[ru] > 0;
  }
  if (!__syncthreads_or(any)) return;
  int32_t ahead = kNoSeen;
  if constexpr (SEEN) {
    // lanes 0 and 1 of a user's kSeenAhead: the first entry of the row not below v_begin, and not below v_end
    const int rl = wv * kRankUsers + lane / kSeenAhead, e = lane % kSeenAhead;
    if (e < 2) {
      int64_t lo = 0, hi = 0;
      if (u0 + rl < nU && tptr[u0 + rl + 1] - tptr[u0 + rl] > first) {  // no threshold: nothing of the row is ever looked at
        lo = sptr[u0 + rl];
        hi = sptr[u0 + rl + 1];
      }
      const int64_t want = e ? v_end : v_begin;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sidx[mid] < want) lo = mid + 1; else hi = mid;
      }
      curs[2 * rl + e] = lo;
    }
    wave_lds_fence();
    ahead = seen_ahead(sidx, curs, wv, lane);
  }
  CrossStage g;
  stage_load(g, qU, qV, Kq, u0, nU, v_begin, nV, 0);
  for (int64_t v0 = v_begin; v0 < v_end; v0 += kCrossTV) {
    v4d_t acc[2];
    cross_tile(qU, qV, Kq, u0, nU, v0, nV, v0 + kCrossTV < v_end ? v0 + kCrossTV : -1, As, Bs, g, acc);
    __syncthreads();  // the item rows have been read: their place takes the scores
    {
      const int cl = 16 * wv + (lane & 15);
      const int64_t col = v0 + cl;
      const double c = col < nV ? cV[col] : 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = 16 * h + (lane >> 4) + 4 * r;
          const double a = u0 + rl < nU ? aU[u0 + rl] : 0.0;
          Sc[rl * kCrossSLD + cl] = cross_score(a, c, acc[h][r]);
        }
    }
    __syncthreads();
    const unsigned long long in_all = SEEN ? __ballot((int64_t)ahead < v0 + kCrossTV) : 0ull;
    const int64_t j = v0 + lane;
#pragma unroll
    for (int ru = 0; ru < kRankUsers; ++ru) {
      if (th[ru] == 0) continue;  // (the rows past nU among them)
      const int rl = wv * kRankUsers + ru;
      const uint64_t key = rank_key((uint64_t)__double_as_longlong(Sc[rl * kCrossSLD + lane]));
      bool pass = j < v_end;
      if constexpr (SEEN) {
        const unsigned long long in = in_all & (((1ull << kSeenAhead) - 1) << (ru * kSeenAhead));
        if (in) {  // the same for every lane, and every lane takes part in finding the mask
          const unsigned long long seen = seen_window(sidx, curs, rl, ahead, in, v0, lane);
          pass = pass && !((seen >> lane) & 1);  // a seen item is counted by no threshold
        }
      }
      for (int q = 0; q < th[ru]; ++q) {  // a threshold never counts its own item: ranks_before of a pair with itself is false
        const unsigned long long before = __ballot(pass && ranks_before(key, (int32_t)j, readlane_u64(tkey[ru], q), __builtin_amdgcn_readlane(tid[ru], q)));
        if (lane == q) tcnt[ru] += (uint32_t)__popcll(before);
      }
    }
    if constexpr (SEEN) {
      if (in_all && v0 + kCrossTV < v_end) {  // a cursor moved: the entries ahead of the next tile, in flight across its product
        wave_lds_fence();
        ahead = seen_ahead(sidx, curs, wv, lane);
      }
    }
    // (cross_tile opens with a barrier: the scores have been read before the next tile's rows are staged)
  }
#pragma unroll
  for (int ru = 0; ru < kRankUsers; ++ru)
    if (lane < th[ru] && tcnt[ru])  // (th > 0: the user exists) integer sums: any order of the chunks, one result
      atomicAdd(cnt + tptr[u0 + wv * kRankUsers + ru] + first + lane, tcnt[ru]);
}

// the longest row, for the number of passes
__global__ void k_max_row_len(int64_t n, const int64_t* __restrict__ indptr, unsigned long long* __restrict__ out) {
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, (unsigned long long)(indptr[i + 1] - indptr[i]));
  for (int s = 1; s < kWave; s <<= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, s, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicMax(out, m);
}

// One lane per held-out entry: its count as int64, or -1 where its item is stored in the user's (ascending) seen row.
__global__ __launch_bounds__(kBlock) void k_rank_of_close(int64_t nU, int64_t nnz, const int64_t* __restrict__ tptr, const int32_t* __restrict__ tidx,
                                                          const uint32_t* __restrict__ cnt, const int64_t* __restrict__ sptr,
                                                          const int32_t* __restrict__ sidx, int64_t* __restrict__ ranks) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
    bool seen = false;
    if (sptr) {
      int64_t lo = 0, hi = nU - 1;  // the last row that starts at or before e: tptr[nU] = nnz > e, so that row holds e
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (tptr[mid] <= e) lo = mid; else hi = mid - 1;
      }
      const int32_t id = tidx[e];
      int64_t a = sptr[lo], b = sptr[lo + 1];
      const int64_t end = b;
      while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (sidx[mid] < id) a = mid + 1; else b = mid;
      }
      seen = a < end && sidx[a] == id;
    }
    ranks[e] = seen ? -1 : (int64_t)cnt[e];
  }
}

// One wavefront per user: nV minus the distinct ids of the ascending seen row (sptr null: nV).
__global__ __launch_bounds__(kBlock) void k_rank_of_candidates(int64_t nU, int64_t nV, const int64_t* __restrict__ sptr, const int32_t* __restrict__ sidx,
                                                               int64_t* __restrict__ n_cand) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nU; u += nwaves) {
    int64_t distinct = 0;
    if (sptr) {
      const int64_t b = sptr[u], e = sptr[u + 1];
      for (int64_t p0 = b; p0 < e; p0 += kWave) {
        const int64_t p = p0 + lane;
        distinct += __popcll(__ballot(p < e && (p == b || sidx[p - 1] != sidx[p])));
      }
    }
    if (lane == 0) n_cand[u] = nV - distinct;
  }
}

}  // namespace

int cross_sides(nfm_ctx* ctx, const CsrView& U, const CsrView& V, const ModelView& M, CrossSides* S) {
  NFM_CHECK(M.kind == NFM_KIND_FM && M.degree == 2 && M.nb == M.kc && M.Kp == 2 * M.L, NFM_ERR_UNSUPPORTED,
            "crossDecisionFunction takes a degree-2 FactorizationMachine");
  S->nU = U.n;
  S->nV = V.n;
  const int kq = M.nb * M.Kp;
  S->Kq = kq < 4 ? 4 : (kq + 3) / 4 * 4;
  NFM_TRY(S->qU.alloc(sizeof(double) * (size_t)std::max<int64_t>(U.n, 1) * S->Kq));
  NFM_TRY(S->qV.alloc(sizeof(double) * (size_t)std::max<int64_t>(V.n, 1) * S->Kq));
  NFM_TRY(S->aU.alloc(sizeof(double) * (size_t)std::max<int64_t>(U.n, 1)));
  NFM_TRY(S->cV.alloc(sizeof(double) * (size_t)std::max<int64_t>(V.n, 1)));
  if (S->Kq != kq) {  // one lane per row (k <= 2): the padding factors are zero
    NFM_HIP_CHECK(hipMemsetAsync(S->qU.p, 0, S->qU.bytes, ctx->stream));
    NFM_HIP_CHECK(hipMemsetAsync(S->qV.p, 0, S->qV.bytes, ctx->stream));
  }
  CsrView Xu = U, Xv = V;
  Xu.d = M.d;  // where the dummy feature's row is (fm_device.h: row_entry)
  TimedLaunch tl(ctx, "cross_side");
  if (U.n > 0)
    NFM_TRY(with_lanes(M.L, [&](auto L) { return launch_side_L<L()>(ctx, Xu, M, 0, M.n_aug, 1, S->Kq, S->qU.as<double>(), S->aU.as<double>()); }));
  if (V.n > 0)
    NFM_TRY(with_lanes(M.L, [&](auto L) { return launch_side_L<L()>(ctx, Xv, M, U.d, 0, 0, S->Kq, S->qV.as<double>(), S->cV.as<double>()); }));
  return NFM_OK;
}

int cross_sides_ffm(nfm_ctx* ctx, const CsrView& U, const CsrView& V, const ModelView& M, CrossSides* S) {
  static const char* kWay = "materialise the pairs, hstack(U[rep], V[tile]), and call decisionFunction";
  NFM_CHECK(M.kind == NFM_KIND_FFM && U.fields && V.fields && U.n_fields >= 1 && V.n_fields >= 1 && U.n_fields + V.n_fields == M.nb, NFM_ERR_INVALID,
            "Invalid nFields.");
  NFM_CHECK(M.Kp == 2 * M.L, NFM_ERR_UNSUPPORTED, "newRanker: field-aware models with n_components > 128 are not served: %s", kWay);
  const int FU = U.n_fields, FV = V.n_fields;
  const int64_t kq = (int64_t)FU * FV * M.Kp;
  NFM_CHECK(kq <= kFfmMaxKq, NFM_ERR_UNSUPPORTED,
            "newRanker: %d x %d fields of %d (padded) factors are %lld sums per row, more than %d: %s", FU, FV, (int)M.Kp, (long long)kq, kFfmMaxKq, kWay);
  S->nU = U.n;
  S->nV = V.n;
  S->Kq = (int)((kq + 3) / 4 * 4);
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = ((double)U.n + (double)V.n) * (S->Kq + 1) * sizeof(double);
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "newRanker: the two sides take %.0f MB (%d doubles per row) and %.0f MB are free: rank row slices of U, or %s", bytes / 1e6, S->Kq,
            (double)mem_free / 1e6, kWay);
  NFM_TRY(S->qU.alloc(sizeof(double) * (size_t)std::max<int64_t>(U.n, 1) * S->Kq));
  NFM_TRY(S->qV.alloc(sizeof(double) * (size_t)std::max<int64_t>(V.n, 1) * S->Kq));
  NFM_TRY(S->aU.alloc(sizeof(double) * (size_t)std::max<int64_t>(U.n, 1)));
  NFM_TRY(S->cV.alloc(sizeof(double) * (size_t)std::max<int64_t>(V.n, 1)));
  int lgL = 0;
  while ((1 << lgL) < M.L) ++lgL;
  const FfmSide su{0, M.nb, 0, FU, FV, FU, FV, lgL, S->Kq}, sv{U.d, M.nb, FU, FV, FU, 0, FV, lgL, S->Kq};
  TimedLaunch tl(ctx, "cross_side_ffm");
  if (U.n > 0) NFM_TRY(launch_side_ffm_T<false>(ctx, U, M, su, S->qU.as<double>(), S->aU.as<double>()));
  if (V.n > 0) NFM_TRY(launch_side_ffm_T<true>(ctx, V, M, sv, S->qV.as<double>(), S->cV.as<double>()));
  return NFM_OK;
}

int cross_scores(nfm_ctx* ctx, const CrossSides& S, int64_t u_begin, int64_t u_end, double* out_dev) {
  if (u_end <= u_begin || S.nV == 0) return NFM_OK;
  const int64_t vt = (S.nV + kCrossTV - 1) / kCrossTV;
  NFM_CHECK(vt <= 2147483647, NFM_ERR_UNSUPPORTED, "crossDecisionFunction: too many items for one launch");
  TimedLaunch tl(ctx, "cross_scores");
  const int64_t rows_per_launch = (int64_t)65535 * kCrossTU;
  for (int64_t b = u_begin; b < u_end; b += rows_per_launch) {
    const int64_t e = std::min(u_end, b + rows_per_launch);
    const unsigned ut = (unsigned)((e - b + kCrossTU - 1) / kCrossTU);
    hipLaunchKernelGGL(k_cross_scores, dim3((unsigned)vt, ut), dim3(kBlock), 0, ctx->stream, S.qU.as<double>(), S.qV.as<double>(), S.aU.as<double>(),
                       S.cV.as<double>(), S.Kq, b, e, S.nV, out_dev + (size_t)(b - u_begin) * S.nV);
    NFM_HIP_CHECK(hipGetLastError());
  }
  return NFM_OK;
}

// the chunk of items one workgroup walks: whole tiles; the library's choice (chunk_items == 0) keeps four workgroups per CU
// busy when there are few users
static int64_t cross_chunk_tiles(nfm_ctx* ctx, const CrossSides& S, int64_t chunk_items) {
  const int64_t tiles_v = (S.nV + kCrossTV - 1) / kCrossTV, tiles_u = (S.nU + kCrossTU - 1) / kCrossTU;
  int64_t chunk_tiles;
  if (chunk_items > 0) {
    chunk_tiles = (chunk_items + kCrossTV - 1) / kCrossTV;
  } else {
    const int64_t want = ((int64_t)ctx->n_cu * 4 + tiles_u - 1) / tiles_u;
    chunk_tiles = (tiles_v + want - 1) / want;
  }
  return std::max<int64_t>(1, std::min(chunk_tiles, tiles_v));
}

int cross_topk(nfm_ctx* ctx, const CrossSides& S, int64_t K, int64_t chunk_items, int64_t* ids_dev, double* scores_dev, const AscendingRows* seen) {
  if (S.nU == 0) return NFM_OK;
  NFM_CHECK(K >= 1 && K <= kCrossMaxTopK && K <= S.nV && S.nV < kNoItem, NFM_ERR_INVALID, "topK out of range");
  NFM_CHECK(!seen || S.nV <= kNoSeen - kCrossTV, NFM_ERR_UNSUPPORTED, "recommend with seen items: too many items");  // a tile's window stays below kNoSeen
  const int64_t tiles_v = (S.nV + kCrossTV - 1) / kCrossTV;
  const int64_t chunk_tiles = cross_chunk_tiles(ctx, S, chunk_items), chunks = (tiles_v + chunk_tiles - 1) / chunk_tiles;
  const size_t lds = (size_t)kCrossTU * K * (sizeof(uint64_t) + sizeof(int32_t)) + (seen ? kSeenLds : 0);
  const void* kernel = seen ? reinterpret_cast<const void*>(k_cross_topk<true>) : reinterpret_cast<const void*>(k_cross_topk<false>);
  if (lds + sizeof(double) * (kCrossTU + kCrossTV) * kCrossLD > 65536)  // beyond the default 64 KiB of a workgroup (K > 102)
    NFM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t rows_per_launch = (int64_t)65535 * kCrossTU;
  const int64_t block_rows = std::min(S.nU, rows_per_launch);
  NFM_CHECK(chunks <= 2147483647, NFM_ERR_UNSUPPORTED, "recommend: %lld chunks of items are too many (chunkItems = %lld)", (long long)chunks,
            (long long)chunk_items);
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double list_bytes = (double)block_rows * (double)chunks * (double)K * (sizeof(uint64_t) + sizeof(int32_t));
  NFM_CHECK(list_bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "recommend: the lists of %lld chunks of items take %.0f MB and %.0f MB are free: pass a larger chunkItems (%lld), or 0 for the "
            "library's choice", (long long)chunks, list_bytes / 1e6, (double)mem_free / 1e6, (long long)chunk_items);
  DevBuf pbits, pids;
  NFM_TRY(pbits.alloc(sizeof(uint64_t) * (size_t)(block_rows * chunks * K)));
  NFM_TRY(pids.alloc(sizeof(int32_t) * (size_t)(block_rows * chunks * K)));
  for (int64_t b = 0; b < S.nU; b += rows_per_launch) {
    const int64_t n = std::min(S.nU - b, rows_per_launch);
    const dim3 grid((unsigned)chunks, (unsigned)((n + kCrossTU - 1) / kCrossTU));
    if (!seen) {
      TimedLaunch tl(ctx, "cross_topk");
      hipLaunchKernelGGL(k_cross_topk<false>, grid, dim3(kBlock), lds, ctx->stream, S.qU.as<double>() + (size_t)b * S.Kq, S.qV.as<double>(),
                         S.aU.as<double>() + b, S.cV.as<double>(), S.Kq, n, S.nV, chunk_tiles * kCrossTV, (int)K, pbits.as<uint64_t>(),
                         pids.as<int32_t>(), nullptr, nullptr);
      NFM_HIP_CHECK(hipGetLastError());
    } else {
      TimedLaunch tl(ctx, "cross_topk_seen");
      hipLaunchKernelGGL(k_cross_topk<true>, grid, dim3(kBlock), lds, ctx->stream, S.qU.as<double>() + (size_t)b * S.Kq, S.qV.as<double>(),
                         S.aU.as<double>() + b, S.cV.as<double>(), S.Kq, n, S.nV, chunk_tiles * kCrossTV, (int)K, pbits.as<uint64_t>(),
                         pids.as<int32_t>(), seen->indptr + b, seen->indices);
      hipLaunchKernelGGL(k_cross_no_item, dim3((unsigned)std::min<int64_t>((n * K + kBlock - 1) / kBlock, (int64_t)ctx->n_cu * 32)), dim3(kBlock), 0,
                         ctx->stream, n * K, ids_dev + (size_t)b * K, scores_dev + (size_t)b * K);
      NFM_HIP_CHECK(hipGetLastError());
    }
    {
      TimedLaunch tl(ctx, "cross_merge");
      int64_t blocks = (n * chunks * K + kBlock - 1) / kBlock;
      blocks = std::min<int64_t>(blocks, (int64_t)ctx->n_cu * 32);
      hipLaunchKernelGGL(k_cross_merge, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, pbits.as<uint64_t>(), pids.as<int32_t>(), n, (int)chunks,
                         (int)K, ids_dev + (size_t)b * K, scores_dev + (size_t)b * K);
      NFM_HIP_CHECK(hipGetLastError());
    }
  }
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the lists go back to the block cache: nothing queued may still read them
  return NFM_OK;
}

int ascending_rows(nfm_ctx* ctx, const CsrView& X, bool rows_ascend, DevBuf* k0, DevBuf* k1, AscendingRows* out) {
  out->indptr = X.indptr;
  out->indices = X.indices;
  if (rows_ascend || X.n == 0 || X.nnz < 2) return NFM_OK;
  return sort_row_ids(ctx, X, k0, k1, &out->indices);
}

int cross_pairs(nfm_ctx* ctx, const CrossSides& S, const int64_t* indptr, const int32_t* indices, int64_t nnz, double* out_dev) {
  if (S.nU == 0 || nnz == 0) return NFM_OK;
  hipStream_t st = ctx->stream;
  DevBuf cnt, blk;
  NFM_TRY(cnt.alloc(sizeof(int64_t) * (size_t)(S.nU + 1)));
  NFM_TRY(blk.alloc(sizeof(int64_t) * (size_t)(S.nU + 1)));
  hipLaunchKernelGGL(k_pair_block_counts, dim3((unsigned)std::min<int64_t>((S.nU + kBlock) / kBlock, (int64_t)ctx->n_cu * 8)), dim3(kBlock), 0, st, S.nU,
                     indptr, cnt.as<int64_t>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(dsop_exclusive_scan(st, cnt.as<int64_t>(), blk.as<int64_t>(), S.nU + 1));
  int64_t nB = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&nB, blk.as<int64_t>() + S.nU, sizeof(nB), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  {
    TimedLaunch tl(ctx, "cross_pairs");
    // four workgroups a CU, what the kernel's registers let reside: 16 wavefronts with a step of 16 rows each in flight; a
    // longer list is walked with that stride
    const int64_t blocks = std::min<int64_t>((nB + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ctx->n_cu * 4);
    hipLaunchKernelGGL(k_cross_pairs, dim3((unsigned)blocks), dim3(kBlock), 0, st, S.qU.as<double>(), S.qV.as<double>(), S.aU.as<double>(),
                       S.cV.as<double>(), S.Kq, S.nU, nB, blk.as<int64_t>(), indptr, indices, out_dev);
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // the block list goes back to the block cache: nothing queued may still read it
  return NFM_OK;
}

int cross_topk_among(nfm_ctx* ctx, const CrossSides& S, const AscendingRows& C, int64_t nnz, int64_t K, int64_t* ids_dev, double* scores_dev) {
  if (S.nU == 0) return NFM_OK;
  NFM_CHECK(K >= 1 && K <= kCrossMaxTopK && K <= S.nV && S.nV < kNoItem, NFM_ERR_INVALID, "topK out of range");
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = (double)nnz * sizeof(double) + (double)(S.nU + 1) * 2.0 * sizeof(int64_t);
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "recommendAmong: the scores of %lld candidates take %.0f MB and %.0f MB are free: rank row slices of U", (long long)nnz, bytes / 1e6,
            (double)mem_free / 1e6);
  DevBuf sc;
  NFM_TRY(sc.alloc(sizeof(double) * (size_t)std::max<int64_t>(nnz, 1)));
  NFM_TRY(cross_pairs(ctx, S, C.indptr, C.indices, nnz, sc.as<double>()));  // of the ascending rows: sc is aligned with what the ranking walks
  {
    TimedLaunch tl(ctx, "cross_rank_among");
    const int64_t blocks = std::min<int64_t>((S.nU + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ctx->n_cu * 32);
    const size_t lds = (size_t)kWavesPerBlock * K * (sizeof(uint64_t) + sizeof(int32_t));
    hipLaunchKernelGGL(k_cross_rank_among, dim3((unsigned)blocks), dim3(kBlock), lds, ctx->stream, S.nU, (int)K, C.indptr, C.indices, sc.as<double>(),
                       ids_dev, scores_dev);
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the scores go back to the block cache
  return NFM_OK;
}

int cross_rank_of(nfm_ctx* ctx, const CrossSides& S, const int64_t* tptr, const int32_t* tidx, int64_t nnz, const AscendingRows* seen, int64_t chunk_items,
                  int64_t* ranks_dev, int64_t* n_cand_dev) {
  if (S.nU == 0) return NFM_OK;
  NFM_CHECK(S.nV < kNoItem && (!seen || S.nV <= kNoSeen - kCrossTV), NFM_ERR_UNSUPPORTED, "rankOf: too many items");
  hipStream_t st = ctx->stream;
  const int64_t* sptr = seen ? seen->indptr : nullptr;
  const int32_t* sidx = seen ? seen->indices : nullptr;
  {
    TimedLaunch tl(ctx, "rank_of_candidates");
    const int64_t blocks = std::min<int64_t>((S.nU + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ctx->n_cu * 32);
    hipLaunchKernelGGL(k_rank_of_candidates, dim3((unsigned)blocks), dim3(kBlock), 0, st, S.nU, S.nV, sptr, sidx, n_cand_dev);
    NFM_HIP_CHECK(hipGetLastError());
  }
  if (nnz == 0) return NFM_OK;  // (nV == 0 among them: no id is below it)
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = (double)nnz * (sizeof(double) + sizeof(uint32_t)) + (double)(S.nU + 1) * 2.0 * sizeof(int64_t);
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "rankOf: the thresholds of %lld held-out entries take %.0f MB and %.0f MB are free: rank row slices of U", (long long)nnz, bytes / 1e6,
            (double)mem_free / 1e6);
  DevBuf thr, cnt, longest;
  NFM_TRY(thr.alloc(sizeof(double) * (size_t)nnz));
  NFM_TRY(cnt.alloc(sizeof(uint32_t) * (size_t)nnz));
  NFM_TRY(longest.alloc(sizeof(unsigned long long)));
  NFM_HIP_CHECK(hipMemsetAsync(cnt.p, 0, cnt.bytes, st));
  NFM_HIP_CHECK(hipMemsetAsync(longest.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_max_row_len, dim3((unsigned)std::min<int64_t>((S.nU + kBlock - 1) / kBlock, (int64_t)ctx->n_cu * 8)), dim3(kBlock), 0, st, S.nU, tptr,
                     longest.as<unsigned long long>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(cross_pairs(ctx, S, tptr, tidx, nnz, thr.as<double>()));  // the thresholds: the bits cross_scores has for the held-out pairs
  unsigned long long row_max = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&row_max, longest.p, sizeof(row_max), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t passes = ((int64_t)row_max + kWave - 1) / kWave;  // >= 1: nnz > 0
  const int64_t tiles_v = (S.nV + kCrossTV - 1) / kCrossTV;
  const int64_t chunk_tiles = cross_chunk_tiles(ctx, S, chunk_items), chunks = (tiles_v + chunk_tiles - 1) / chunk_tiles;
  NFM_CHECK(chunks <= 2147483647, NFM_ERR_UNSUPPORTED, "rankOf: %lld chunks of items are too many (chunkItems = %lld)", (long long)chunks,
            (long long)chunk_items);
  const int64_t rows_per_launch = (int64_t)65535 * kCrossTU, passes_per_launch = 65535;
  {
    TimedLaunch tl(ctx, seen ? "cross_rank_of_seen" : "cross_rank_of");
    for (int64_t b = 0; b < S.nU; b += rows_per_launch)
      for (int64_t p0 = 0; p0 < passes; p0 += passes_per_launch) {
        const int64_t n = std::min(S.nU - b, rows_per_launch);
        const dim3 grid((unsigned)chunks, (unsigned)((n + kCrossTU - 1) / kCrossTU), (unsigned)std::min(passes - p0, passes_per_launch));
        if (seen)
          hipLaunchKernelGGL(k_cross_rank_of<true>, grid, dim3(kBlock), 0, st, S.qU.as<double>() + (size_t)b * S.Kq, S.qV.as<double>(), S.aU.as<double>() + b,
                             S.cV.as<double>(), S.Kq, n, S.nV, chunk_tiles * kCrossTV, tptr + b, tidx, thr.as<double>(), p0, cnt.as<uint32_t>(), sptr + b, sidx);
        else
          hipLaunchKernelGGL(k_cross_rank_of<false>, grid, dim3(kBlock), 0, st, S.qU.as<double>() + (size_t)b * S.Kq, S.qV.as<double>(), S.aU.as<double>() + b,
                             S.cV.as<double>(), S.Kq, n, S.nV, chunk_tiles * kCrossTV, tptr + b, tidx, thr.as<double>(), p0, cnt.as<uint32_t>(), nullptr, nullptr);
        NFM_HIP_CHECK(hipGetLastError());
      }
  }
  {
    TimedLaunch tl(ctx, "rank_of_close");
    const int64_t blocks = std::min<int64_t>((nnz + kBlock - 1) / kBlock, (int64_t)ctx->n_cu * 32);
    hipLaunchKernelGGL(k_rank_of_close, dim3((unsigned)blocks), dim3(kBlock), 0, st, S.nU, nnz, tptr, tidx, cnt.as<uint32_t>(), sptr, sidx, ranks_dev);
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // the thresholds and counts go back to the block cache
  return NFM_OK;
}

int cross_rank_metrics(nfm_ctx* ctx, int64_t nU, int64_t K, const int64_t* ids_dev, const AscendingRows& T, double out[5]) {
  NFM_CHECK(K >= 1 && K <= kCrossMaxTopK, NFM_ERR_INVALID, "topK out of range");
  double tab[2 * kCrossMaxTopK];  // disc[r] = 1 / log2(r + 2), and its prefix sums by ascending r
  double run = 0.0;
  for (int r = 0; r < kCrossMaxTopK; ++r) {
    tab[r] = 1.0 / log2((double)r + 2.0);
    tab[kCrossMaxTopK + r] = run += tab[r];
  }
  DevBuf tab_dev, per, res;
  NFM_TRY(tab_dev.alloc(sizeof(tab)));
  NFM_TRY(per.alloc(sizeof(double) * 5 * (size_t)std::max<int64_t>(nU, 1)));
  NFM_TRY(res.alloc(sizeof(double) * 5));
  NFM_HIP_CHECK(hipMemcpyAsync(tab_dev.p, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // tab is this frame's
  {
    TimedLaunch tl(ctx, "cross_rank_metrics");
    if (nU > 0) {
      const int64_t blocks = std::min<int64_t>((nU + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ctx->n_cu * 32);
      hipLaunchKernelGGL(k_rank_metrics, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, nU, (int)K, ids_dev, T.indptr, T.indices,
                         tab_dev.as<double>(), tab_dev.as<double>() + kCrossMaxTopK, per.as<double>());
    }
    hipLaunchKernelGGL(k_rank_metrics_fold, dim3(1), dim3(kWave), 0, ctx->stream, nU, per.as<double>(), res.as<double>());
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipMemcpyAsync(out, res.p, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return NFM_OK;
}

}  // namespace nfm
