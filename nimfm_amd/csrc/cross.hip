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
// The bits of a score depend on its two rows and the model alone: every output of the matrix instruction is its own chain
// over the factors, edge tiles run on zero operands, and a row's scalar is added the same way wherever the row stands.
// No kernel waits for another workgroup, a flag in memory or the host.
#include <algorithm>

#include "cross.h"
#include "fm_device.h"

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

// what one wavefront has written to LDS is what its lanes read next
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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

// grid: x = item chunk, y = user tile.  pbits / pids [nU][chunks][K].
__global__ __launch_bounds__(kBlock) void k_cross_topk(const double* __restrict__ qU, const double* __restrict__ qV, const double* __restrict__ aU,
                                                       const double* __restrict__ cV, int Kq, int64_t nU, int64_t nV, int64_t chunk_len, int K,
                                                       uint64_t* __restrict__ pbits, int32_t* __restrict__ pids) {
  __shared__ __attribute__((aligned(16))) double As[kCrossTU * kCrossLD];
  __shared__ __attribute__((aligned(16))) double Bs[kCrossTV * kCrossLD];
  extern __shared__ __attribute__((aligned(16))) unsigned char cross_dyn[];
  uint64_t* lbits = reinterpret_cast<uint64_t*>(cross_dyn);                  // [kCrossTU][K]
  int32_t* lids = reinterpret_cast<int32_t*>(lbits + (size_t)kCrossTU * K);  // [kCrossTU][K]
  double* Sc = Bs;  // the tile of scores, [kCrossTU][kCrossSLD], once the item rows have been used
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const int64_t u0 = (int64_t)blockIdx.y * kCrossTU;
  const int64_t v_begin = (int64_t)blockIdx.x * chunk_len, v_end = v_begin + chunk_len < nV ? v_begin + chunk_len : nV;
  for (int p = t; p < kCrossTU * K; p += kBlock) {
    lbits[p] = 0x7ff8000000000000ull;
    lids[p] = kNoItem;
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
    for (int ru = 0; ru < kCrossTU / kWavesPerBlock; ++ru) {
      const int rl = wv * (kCrossTU / kWavesPerBlock) + ru;
      if (u0 + rl >= nU) break;
      uint64_t* lb = lbits + (size_t)rl * K;
      int32_t* li = lids + (size_t)rl * K;
      const int64_t j = v0 + lane;
      const uint64_t bits = (uint64_t)__double_as_longlong(Sc[rl * kCrossSLD + lane]);
      const uint64_t key = rank_key(bits);
      const bool pass = j < v_end && ranks_before(key, (int32_t)j, rank_key(lb[K - 1]), li[K - 1]);
      unsigned long long mask = __ballot(pass);
      while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const uint64_t cbits = (uint64_t)__shfl((long long)bits, src, kWave);
        const int32_t cid = (int32_t)(v0 + src);
        if (ranks_before(rank_key(cbits), cid, rank_key(lb[K - 1]), li[K - 1])) list_insert(lb, li, K, cbits, cid, lane);
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

int cross_topk(nfm_ctx* ctx, const CrossSides& S, int64_t K, int64_t chunk_items, int64_t* ids_dev, double* scores_dev) {
  if (S.nU == 0) return NFM_OK;
  NFM_CHECK(K >= 1 && K <= kCrossMaxTopK && K <= S.nV && S.nV < kNoItem, NFM_ERR_INVALID, "topK out of range");
  const int64_t tiles_v = (S.nV + kCrossTV - 1) / kCrossTV, tiles_u = (S.nU + kCrossTU - 1) / kCrossTU;
  // the chunk: whole tiles; the library's choice keeps four workgroups per CU busy when there are few users
  int64_t chunk_tiles;
  if (chunk_items > 0) {
    chunk_tiles = (chunk_items + kCrossTV - 1) / kCrossTV;
  } else {
    const int64_t want = ((int64_t)ctx->n_cu * 4 + tiles_u - 1) / tiles_u;
    chunk_tiles = (tiles_v + want - 1) / want;
  }
  chunk_tiles = std::max<int64_t>(1, std::min(chunk_tiles, tiles_v));
  const int64_t chunks = (tiles_v + chunk_tiles - 1) / chunk_tiles;
  const size_t lds = (size_t)kCrossTU * K * (sizeof(uint64_t) + sizeof(int32_t));
  if (lds + sizeof(double) * (kCrossTU + kCrossTV) * kCrossLD > 65536)  // beyond the default 64 KiB of a workgroup (K > 102)
    NFM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_cross_topk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
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
    {
      TimedLaunch tl(ctx, "cross_topk");
      hipLaunchKernelGGL(k_cross_topk, dim3((unsigned)chunks, (unsigned)((n + kCrossTU - 1) / kCrossTU)), dim3(kBlock), lds, ctx->stream,
                         S.qU.as<double>() + (size_t)b * S.Kq, S.qV.as<double>(), S.aU.as<double>() + b, S.cV.as<double>(), S.Kq, n, S.nV,
                         chunk_tiles * kCrossTV, (int)K, pbits.as<uint64_t>(), pids.as<int32_t>());
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

}  // namespace nfm
