// nimfm_amd/csrc/interactions.hip -- the interaction matrix of a fitted FM reduced where it is made (interactions.h, DESIGN.md
// section 36).
//   k_inter_sig     per row j of Q = P[order]^T (ModelView::row, the kc blocks side by side, the lazy scale applied): the 64-bit
//                   signature of its non-zero factors; a row with none is dropped
//   k_inter_rows    the kept rows, at the places an exclusive scan gives them (ascending by id) -> Qc [dn][Kq], ids, sig
//   k_inter_tsig    the OR of the signatures of the kInterT rows of a tile
//   inter_tile      a kInterT x kInterT block of Qc diag(lams) Qc^T on v_mfma_f64_16x16x4_f64: both operands are rows of Qc, a
//                   diagonal tile stages its rows once; the next step's rows (or the next live tile's first step) are in flight
//   k_inter_stats   the upper triangle of tiles, one tile per trip: sum |w| over i < j and over i == j, the pairs i < j with
//                   w != 0 (ballot + popcount), the "used" flag of both features; a tile whose signatures are disjoint is skipped
//   k_inter_fold    the per-tile sums added in one fixed order, the flags counted
//   k_inter_topk    the same walk over a chunk of tiles: the K best (|w|, i, j) of the chunk in one sorted list in LDS
//   k_inter_merge   the chunks' lists -> the K best, by rank (the ranks are distinct: the pairs are)
// Every number depends on the model alone: a tile's sums are reduced lane -> wave -> workgroup in a fixed order and stored per
// tile, the fold's order is a function of the tile count, the counts are integers added the same way, and a total order ranks
// the pairs.  There are no floating-point atomics.  No kernel waits for another workgroup, a flag in memory or the host.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "dataset_ops.h"
#include "fm_device.h"
#include "interactions.h"

namespace nfm {

namespace {

typedef double v4d_t __attribute__((ext_vector_type(4)));

constexpr int kInterLD = kInterKS + 2;  // doubles per staged row: 16 rows x 2 factors of a half wave fall into 32 different 8-byte banks (cross.hip)
constexpr int kInterSLD = kInterT + 1;  // doubles per row of the tile of weights
constexpr int kInterSub = 4;            // lanes per row of Q in the compaction
constexpr uint64_t kNoPair = ~0ull;     // the pair of an empty list slot: ranks below every pair
constexpr uint64_t kNanBits = 0x7ff8000000000000ull;
static_assert(kBlock == 256 && kInterT == 64 && kInterKS == 32, "the staging and the wave -> subtile map below are written for these");
static_assert(kInterT * kInterSLD <= 2 * kInterT * kInterLD, "the tile of weights reuses the staged rows");

__device__ __forceinline__ void wave_lds_fence() {  // what one wavefront has written to LDS is what its lanes read next
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the rows of Q that are not all zero ----
// word p of row j: the factors 2 p, 2 p + 1 of the order's kc * Kp; kInterSub lanes share a row
__device__ __forceinline__ double2 q_word(const dev::PlainParams& ps, const ModelView& M, int order, int64_t j, int p) {
  const int hw = M.Kp / 2, c = p / hw, off = p - c * hw;
  return ps.load(M.row((int64_t)order * M.kc + c, j) * M.Kp + 2 * (size_t)off);
}

// rowsig [da], cnt [da + 1] (1 for a kept row; the last one 0: the scan's total lands there)
__global__ __launch_bounds__(kBlock) void k_inter_sig(ModelView M, int order, uint64_t* __restrict__ rowsig, int64_t* __restrict__ cnt) {
  const dev::PlainParams ps{M.P, M.sc[SC_SCALE_P]};
  const int sub = threadIdx.x % kInterSub, words = M.kc * M.Kp / 2;
  const int64_t rows_per_grid = (int64_t)gridDim.x * (kBlock / kInterSub);
  for (int64_t j0 = (int64_t)blockIdx.x * (kBlock / kInterSub); j0 <= M.da; j0 += rows_per_grid) {  // the same trips for every lane
    const int64_t j = j0 + threadIdx.x / kInterSub;
    unsigned long long s = 0;
    if (j < M.da)
      for (int p = sub; p < words; p += kInterSub) {
        const double2 v = q_word(ps, M, order, j, p);
        if (v.x != 0.0) s |= 1ull << ((2 * p) & 63);  // NaN is not zero; -0 is
        if (v.y != 0.0) s |= 1ull << ((2 * p + 1) & 63);
      }
#pragma unroll
    for (int x = 1; x < kInterSub; x <<= 1) s |= (unsigned long long)__shfl_xor((long long)s, x, kWave);
    if (sub == 0 && j <= M.da) {
      if (j < M.da) rowsig[j] = s;
      cnt[j] = s != 0;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_inter_rows(ModelView M, int order, int Kq, const uint64_t* __restrict__ rowsig, const int64_t* __restrict__ pos,
                                                       double* __restrict__ Qc, int64_t* __restrict__ ids, uint64_t* __restrict__ sig) {
  const dev::PlainParams ps{M.P, M.sc[SC_SCALE_P]};
  const int sub = threadIdx.x % kInterSub, words = M.kc * M.Kp / 2;
  for (int64_t j = (int64_t)blockIdx.x * (kBlock / kInterSub) + threadIdx.x / kInterSub; j < M.da; j += (int64_t)gridDim.x * (kBlock / kInterSub)) {
    const uint64_t s = rowsig[j];
    if (s == 0) continue;
    const int64_t at = pos[j];
    double* dst = Qc + (size_t)at * Kq;
    for (int p = sub; p < words; p += kInterSub) *reinterpret_cast<double2*>(dst + 2 * p) = q_word(ps, M, order, j, p);
    if (sub == 0) {
      if (Kq > 2 * words) *reinterpret_cast<double2*>(dst + 2 * words) = double2{0.0, 0.0};  // Kq is 2 words + 2 at the most
      ids[at] = j;
      sig[at] = s;
    }
  }
}

// one wavefront per tile of rows
__global__ __launch_bounds__(kBlock) void k_inter_tsig(int64_t dn, int64_t nT, const uint64_t* __restrict__ sig, uint64_t* __restrict__ tsig) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t I = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); I < nT; I += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t i = I * kInterT + lane;
    unsigned long long s = i < dn ? sig[i] : 0;
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) s |= (unsigned long long)__shfl_xor((long long)s, x, kWave);
    if (lane == 0) tsig[I] = s;
  }
}

// ---- the upper triangle of tiles ----
// Tile t of nT (nT + 1) / 2, row by row: row I holds the tiles (I, I) .. (I, nT - 1) and starts at tri_start(I).  The root
// gives I to within a place or two; the two loops settle it on integers.
__host__ __device__ __forceinline__ int64_t tri_start(int64_t I, int64_t nT) { return I * nT - I * (I - 1) / 2; }
__host__ __device__ __forceinline__ void tri_tile(int64_t t, int64_t nT, int64_t& I, int64_t& J) {
  const double b = 2.0 * (double)nT + 1.0;
  int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  i = i < 0 ? 0 : i > nT - 1 ? nT - 1 : i;
  while (i > 0 && tri_start(i, nT) > t) --i;
  while (i + 1 < nT && tri_start(i + 1, nT) <= t) ++i;
  I = i;
  J = i + (t - tri_start(i, nT));
}
// the first tile at or after t, in steps of `step`, whose rows and columns share a factor; >= end: none
__device__ __forceinline__ int64_t next_live(int64_t t, int64_t step, int64_t end, int64_t nT, const uint64_t* __restrict__ tsig, int64_t& I, int64_t& J) {
  for (; t < end; t += step) {
    tri_tile(t, nT, I, J);
    if (tsig[I] & tsig[J]) return t;
  }
  return end;
}

struct InterSide {
  const double* Qc;
  const double* lams;
  int64_t dn;
  int Kq, nlam;
};

// One step of kInterKS factors of a tile's rows on their way from global memory to LDS, in registers.
struct InterStage {
  double2 a[4];  // rows of the tile's I side: row t / 4, eight factors from 8 (t % 4)
  double2 b[4];  // of its J side; a diagonal tile has none
  double lam;    // t < kInterKS: lams of factor s0 + t
};
__device__ __forceinline__ void stage_rows(double2 (&v)[4], const InterSide& S, int64_t r0, int s0, int ks) {
  const int t = threadIdx.x, r = t >> 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 8 * (t & 3) + 4 * h;
    v[2 * h] = v[2 * h + 1] = double2{0.0, 0.0};  // rows past dn and factors past Kq are zero operands
    if (r0 + r < S.dn && c < ks) {
      const double* p = S.Qc + (size_t)(r0 + r) * S.Kq + s0 + c;
      v[2 * h] = *reinterpret_cast<const double2*>(p);
      v[2 * h + 1] = *reinterpret_cast<const double2*>(p + 2);
    }
  }
}
__device__ __forceinline__ void stage_load(InterStage& g, const InterSide& S, int64_t I, int64_t J, int s0) {
  const int t = threadIdx.x;
  const int ks = S.Kq - s0 < kInterKS ? S.Kq - s0 : kInterKS;  // a multiple of 4
  stage_rows(g.a, S, I * kInterT, s0, ks);
  if (I != J) stage_rows(g.b, S, J * kInterT, s0, ks);
  g.lam = t < kInterKS && s0 + t < S.nlam ? S.lams[s0 + t] : 0.0;
}
__device__ __forceinline__ void store_rows(const double2 (&v)[4], double* Rs) {
  const int t = threadIdx.x;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    *reinterpret_cast<double2*>(Rs + (t >> 2) * kInterLD + 8 * (t & 3) + 4 * h) = v[2 * h];
    *reinterpret_cast<double2*>(Rs + (t >> 2) * kInterLD + 8 * (t & 3) + 4 * h + 2) = v[2 * h + 1];
  }
}

// acc[h][r] of lane l of wave w: row 16 h + (l >> 4) + 4 r, column 16 w + (l & 15) of tile (I, J) -- the operand and result maps
// of cross.hip's cross_tile, a wave owning four row blocks of one column block.  Ops: 2 kInterT staged rows of kInterLD doubles
// (a diagonal tile uses the first half for both operands), Ls: the step's lams.  The column operand carries lams:
// w_ij = sum_s q_is (lams_s q_js).  g holds the tile's first step on entry and, on return, the first step of tile (In, Jn) if
// `more`.  Every lane of the workgroup calls it; on return the lanes may still be reading Ops (the caller syncs before reuse).
__device__ __forceinline__ void inter_tile(const InterSide& S, int64_t I, int64_t J, bool more, int64_t In, int64_t Jn, double* Ops, double* Ls, InterStage& g,
                                           v4d_t (&acc)[4]) {
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  double* As = Ops;
  double* Bs = I == J ? Ops : Ops + kInterT * kInterLD;
#pragma unroll
  for (int h = 0; h < 4; ++h) acc[h] = v4d_t{0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < S.Kq; s0 += kInterKS) {
    const int ks = S.Kq - s0 < kInterKS ? S.Kq - s0 : kInterKS;
    __syncthreads();  // the last step's operands (and a caller's tile of weights) have been read
    store_rows(g.a, As);
    if (I != J) store_rows(g.b, Bs);
    if (t < kInterKS) Ls[t] = g.lam;
    __syncthreads();
    if (s0 + kInterKS < S.Kq)
      stage_load(g, S, I, J, s0 + kInterKS);
    else if (more)
      stage_load(g, S, In, Jn, 0);
    const int r = lane & 15, f = lane >> 4;
    for (int k4 = 0; k4 < ks; k4 += 4) {
      const double bb = Bs[(16 * wv + r) * kInterLD + k4 + f] * Ls[k4 + f];
#pragma unroll
      for (int h = 0; h < 4; ++h) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(16 * h + r) * kInterLD + k4 + f], bb, acc[h], 0, 0, 0);
    }
  }
}

// part [nTiles][2] and tcount [nTiles], cleared before the launch: a tile's sum of |w| over i < j and over i == j, and its pairs
// i < j with w != 0.  flags [dn], cleared: 1 for a feature in such a pair; a flag that stands is not stored again (every
// tile of a dense model would otherwise store its 128 flags, all to the same few lines).
__global__ __launch_bounds__(kBlock) void k_inter_stats(InterSide S, int64_t nT, int64_t nTiles, const uint64_t* __restrict__ tsig, double* __restrict__ part,
                                                        uint32_t* __restrict__ tcount, int32_t* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) double Ops[2 * kInterT * kInterLD];
  __shared__ double Ls[kInterKS];
  __shared__ double red[kWavesPerBlock][2];
  __shared__ uint32_t redc[kWavesPerBlock];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  int64_t I = 0, J = 0, In = 0, Jn = 0;
  int64_t tile = next_live(blockIdx.x, gridDim.x, nTiles, nT, tsig, I, J);  // the same for every lane
  if (tile >= nTiles) return;
  InterStage g;
  stage_load(g, S, I, J, 0);
  while (tile < nTiles) {
    const int64_t tn = next_live(tile + gridDim.x, gridDim.x, nTiles, nT, tsig, In, Jn);
    v4d_t acc[4];
    inter_tile(S, I, J, tn < nTiles, In, Jn, Ops, Ls, g, acc);
    const bool diag = I == J;
    const int cl = 16 * wv + (lane & 15);
    const int64_t j = J * kInterT + cl;
    double su = 0.0, sd = 0.0;
    uint32_t cnt = 0;
    bool col_used = false;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = 16 * h + (lane >> 4) + 4 * r;
        const int64_t i = I * kInterT + rl;
        const double w = acc[h][r], aw = fabs(w);
        const bool valid = i < S.dn && j < S.dn;
        const bool upper = valid && (!diag || rl < cl);  // i < j
        if (upper) su += aw;
        if (valid && diag && rl == cl) sd += aw;
        const bool nz = upper && w != 0.0;  // -0 is zero, NaN is not
        const unsigned long long m = __ballot(nz);
        cnt += __popcll(m);
        col_used |= nz;
        if ((lane & 15) == 0 && ((m >> (16 * (lane >> 4))) & 0xffffull) && !flags[i]) flags[i] = 1;  // one of the row's 16 columns here
      }
    const unsigned long long cm = __ballot(col_used);  // column c of the wave's 16: the lanes c, c + 16, c + 32, c + 48
    if (lane < 16 && (((cm | (cm >> 16) | (cm >> 32) | (cm >> 48)) >> lane) & 1) && !flags[j]) flags[j] = 1;
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) {
      su += dev::shfl_xor_d(su, x);
      sd += dev::shfl_xor_d(sd, x);
    }
    if (lane == 0) {
      red[wv][0] = su;
      red[wv][1] = sd;
      redc[wv] = cnt;
    }
    __syncthreads();
    if (t < 2) part[2 * tile + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (t == 2) tcount[tile] = redc[0] + redc[1] + redc[2] + redc[3];
    // (inter_tile opens with two barriers before a wave comes back to red)
    tile = tn;
    I = In;
    J = Jn;
  }
}

// One workgroup.  Lane l adds the tiles [l seg, (l + 1) seg), seg = ceil(nTiles / kBlock), by ascending tile; lane 0 adds the
// lanes' sums by ascending lane: an order that the tile count fixes.  res_d: sum |w| over all i, j; over i != j.  res_c: the
// pairs, the features with a flag.
__global__ __launch_bounds__(kBlock) void k_inter_fold(int64_t nTiles, const double* __restrict__ part, int64_t dn, const int32_t* __restrict__ flags,
                                                       const uint32_t* __restrict__ tcount, double* __restrict__ res_d, int64_t* __restrict__ res_c) {
  __shared__ double sums[kBlock][2];
  __shared__ int64_t used[kBlock], found[kBlock];
  const int l = threadIdx.x;
  const int64_t seg = (nTiles + kBlock - 1) / kBlock, lo = std::min<int64_t>(l * seg, nTiles), hi = std::min<int64_t>(lo + seg, nTiles);
  double su = 0.0, sd = 0.0;
  int64_t np = 0;
#pragma unroll 8
  for (int64_t t = lo; t < hi; ++t) {
    su += part[2 * t];
    sd += part[2 * t + 1];
    np += tcount[t];
  }
  int64_t nf = 0;
  for (int64_t i = l; i < dn; i += kBlock) nf += flags[i];
  sums[l][0] = su;
  sums[l][1] = sd;
  used[l] = nf;
  found[l] = np;
  __syncthreads();
  if (l == 0) {
    su = sd = 0.0;
    nf = np = 0;
    for (int x = 0; x < kBlock; ++x) {
      su += sums[x][0];
      sd += sums[x][1];
      nf += used[x];
      np += found[x];
    }
    res_d[0] = 2.0 * su + sd;  // every pair i < j stands in W twice
    res_d[1] = 2.0 * su;
    res_c[0] = np;
    res_c[1] = nf;
  }
}

// ---- ranking ----
// (|w|, i, j) ranks before (|w'|, i', j') if |w| > |w'|, or they are equal and (i, j) < (i', j'); NaN below every number, NaN
// against NaN by pair.  key: the bits of |w| (w != 0), which ascend with it; NaN -> 0.  A pair is i * 2^32 + j.
__device__ __forceinline__ uint64_t abs_key(uint64_t bits) {
  const uint64_t a = bits & 0x7fffffffffffffffull;
  return a > 0x7ff0000000000000ull ? 0 : a;
}
__device__ __forceinline__ bool pair_before(uint64_t key_a, uint64_t pair_a, uint64_t key_b, uint64_t pair_b) {
  return key_a > key_b || (key_a == key_b && pair_a < pair_b);
}

// cross.hip's list_insert on a 64-bit id: K (bits, pair) in LDS, best first, empty slots (NaN, kNoPair) last.  One wavefront
// puts a candidate that ranks before the last entry in its place.
__device__ __forceinline__ void pair_insert(uint64_t* lb, uint64_t* lp, int K, uint64_t cbits, uint64_t cpair, int lane) {
  const uint64_t ckey = abs_key(cbits);
  uint64_t eb[kInterMaxTopK / kWave], ep[kInterMaxTopK / kWave];
  const int rounds = (K + kWave - 1) / kWave;  // the same for every lane
  int pos = 0;
#pragma unroll
  for (int c = 0; c < kInterMaxTopK / kWave; ++c) {
    eb[c] = kNanBits;
    ep[c] = kNoPair;
    if (c < rounds) {
      const int p = lane + c * kWave;
      bool before = false;
      if (p < K) {
        eb[c] = lb[p];
        ep[c] = lp[p];
        before = pair_before(abs_key(eb[c]), ep[c], ckey, cpair);
      }
      pos += __popcll(__ballot(before));
    }
  }
  wave_lds_fence();
#pragma unroll
  for (int c = 0; c < kInterMaxTopK / kWave; ++c) {
    const int p = lane + c * kWave;
    if (c < rounds && p >= pos && p + 1 < K) {
      lb[p + 1] = eb[c];
      lp[p + 1] = ep[c];
    }
  }
  if (lane == 0 && pos < K) {
    lb[pos] = cbits;
    lp[pos] = cpair;
  }
  wave_lds_fence();
}

// grid: x = chunk of chunk_tiles tiles.  pbits / ppairs [chunks][K].  The tile's weights go to LDS; every wave marks, per row,
// the columns that rank before the list's last entry as it stood before the tile (nearly always none); wave 0 puts them in
// place one by one, each compared with the last entry as it stands then.
__global__ __launch_bounds__(kBlock) void k_inter_topk(InterSide S, int64_t nT, int64_t nTiles, int64_t chunk_tiles, const uint64_t* __restrict__ tsig, int K,
                                                       uint64_t* __restrict__ pbits, uint64_t* __restrict__ ppairs) {
  __shared__ __attribute__((aligned(16))) double Ops[2 * kInterT * kInterLD];
  __shared__ double Ls[kInterKS];
  __shared__ unsigned long long passm[kInterT];
  extern __shared__ __attribute__((aligned(16))) unsigned char inter_dyn[];
  uint64_t* lb = reinterpret_cast<uint64_t*>(inter_dyn);  // [K]
  uint64_t* lp = lb + K;                                  // [K]
  double* Sc = Ops;  // the tile of weights, [kInterT][kInterSLD], once the rows have been used
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const int64_t t_begin = (int64_t)blockIdx.x * chunk_tiles, t_end = std::min<int64_t>(t_begin + chunk_tiles, nTiles);
  for (int p = t; p < K; p += kBlock) {
    lb[p] = kNanBits;
    lp[p] = kNoPair;
  }
  int64_t I = 0, J = 0, In = 0, Jn = 0;
  int64_t tile = next_live(t_begin, 1, t_end, nT, tsig, I, J);  // the same for every lane
  InterStage g;
  if (tile < t_end) stage_load(g, S, I, J, 0);
  while (tile < t_end) {
    const int64_t tn = next_live(tile + 1, 1, t_end, nT, tsig, In, Jn);
    v4d_t acc[4];
    inter_tile(S, I, J, tn < t_end, In, Jn, Ops, Ls, g, acc);
    __syncthreads();  // the rows have been read: their place takes the weights
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) Sc[(16 * h + (lane >> 4) + 4 * r) * kInterSLD + 16 * wv + (lane & 15)] = acc[h][r];
    __syncthreads();
    const bool diag = I == J;
    const uint64_t last_key = abs_key(lb[K - 1]), last_pair = lp[K - 1];
    for (int ru = 0; ru < kInterT / kWavesPerBlock; ++ru) {  // wave w marks the rows 16 w .. 16 w + 15, one column per lane
      const int rl = wv * (kInterT / kWavesPerBlock) + ru;
      const int64_t i = I * kInterT + rl, j = J * kInterT + lane;
      const double w = Sc[rl * kInterSLD + lane];
      const bool cand = i < S.dn && j < S.dn && (!diag || rl < lane) && w != 0.0;
      const bool pass = cand && pair_before(abs_key((uint64_t)__double_as_longlong(w)), ((uint64_t)i << 32) | (uint64_t)j, last_key, last_pair);
      const unsigned long long m = __ballot(pass);
      if (lane == 0) passm[rl] = m;
    }
    __syncthreads();
    if (wv == 0) {
      unsigned long long rows = __ballot(passm[lane] != 0);
      while (rows) {
        const int rl = __ffsll(rows) - 1;
        rows &= rows - 1;
        unsigned long long mask = passm[rl];
        while (mask) {
          const int cl = __ffsll(mask) - 1;
          mask &= mask - 1;
          const uint64_t cbits = (uint64_t)__double_as_longlong(Sc[rl * kInterSLD + cl]);
          const uint64_t cpair = ((uint64_t)(I * kInterT + rl) << 32) | (uint64_t)(J * kInterT + cl);
          if (pair_before(abs_key(cbits), cpair, abs_key(lb[K - 1]), lp[K - 1])) pair_insert(lb, lp, K, cbits, cpair, lane);
        }
      }
    }
    // (inter_tile opens with a barrier: the weights and marks have been read before the next tile's rows are staged)
    tile = tn;
    I = In;
    J = Jn;
  }
  __syncthreads();
  for (int p = t; p < K; p += kBlock) {
    pbits[(size_t)blockIdx.x * K + p] = lb[p];
    ppairs[(size_t)blockIdx.x * K + p] = lp[p];
  }
}

// pairs [K][2], weights [K]: a rank that no pair fills
__global__ void k_inter_no_pair(int K, int64_t* __restrict__ pairs, double* __restrict__ weights) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < K; e += gridDim.x * blockDim.x) {
    pairs[2 * e] = pairs[2 * e + 1] = -1;
    weights[e] = __longlong_as_double((long long)kNanBits);
  }
}

// cross.hip's k_cross_merge for one row: a lane per entry of the chunks' lists; its rank is its place in its own list plus, for
// every other list, the entries there that rank before it
__global__ __launch_bounds__(kBlock) void k_inter_merge(const uint64_t* __restrict__ pbits, const uint64_t* __restrict__ ppairs, int64_t chunks, int K,
                                                        const int64_t* __restrict__ ids, int64_t* __restrict__ pairs, double* __restrict__ weights) {
  const int64_t total = chunks * K;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const uint64_t pair = ppairs[e];
    if (pair == kNoPair) continue;
    const int p = (int)(e % K);
    const int64_t c = e / K;
    const uint64_t bits = pbits[e], key = abs_key(bits);
    int64_t rank = p;
    for (int64_t c2 = 0; c2 < chunks && rank < K; ++c2) {
      if (c2 == c) continue;
      const size_t base = (size_t)c2 * K;
      int lo = 0, hi = K;  // the first entry of list c2 that does not rank before this one
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pair_before(abs_key(pbits[base + mid]), ppairs[base + mid], key, pair)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < K) {
      pairs[2 * rank] = ids[pair >> 32];
      pairs[2 * rank + 1] = ids[pair & 0xffffffffull];
      weights[rank] = __longlong_as_double((long long)bits);
    }
  }
}

InterSide side_of(const InterRows& R) { return InterSide{R.Qc.as<double>(), R.lams, R.dn, R.Kq, R.nlam}; }

}  // namespace

int inter_rows(nfm_ctx* ctx, const ModelView& M, int order, InterRows* R) {
  hipStream_t st = ctx->stream;
  const int64_t da = M.da;
  NFM_CHECK(da < 2147483647 - kInterT, NFM_ERR_UNSUPPORTED, "interactionStats: too many features");
  R->nlam = M.kc * M.Kp;
  R->Kq = (R->nlam + 3) / 4 * 4;
  R->lams = M.lams;
  R->dn = 0;
  if (da == 0) return NFM_OK;
  DevBuf rowsig, cnt, pos;
  NFM_TRY(rowsig.alloc(sizeof(uint64_t) * (size_t)da));
  NFM_TRY(cnt.alloc(sizeof(int64_t) * (size_t)(da + 1)));
  NFM_TRY(pos.alloc(sizeof(int64_t) * (size_t)(da + 1)));
  const int rows_per_block = kBlock / kInterSub;
  const unsigned blocks = (unsigned)std::min<int64_t>((da + rows_per_block) / rows_per_block, (int64_t)ctx->n_cu * 32);
  TimedLaunch tl(ctx, "inter_rows");
  hipLaunchKernelGGL(k_inter_sig, dim3(blocks), dim3(kBlock), 0, st, M, order, rowsig.as<uint64_t>(), cnt.as<int64_t>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(dsop_exclusive_scan(st, cnt.as<int64_t>(), pos.as<int64_t>(), da + 1));
  int64_t dn = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&dn, pos.as<int64_t>() + da, sizeof(dn), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  R->dn = dn;
  if (dn == 0) return NFM_OK;
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = (double)dn * (R->Kq * sizeof(double) + sizeof(int64_t) + sizeof(uint64_t));
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "interactionStats: the %lld rows of P^T that are not all zero take %.0f MB (%d factors each) and %.0f MB are free", (long long)dn, bytes / 1e6,
            R->Kq, (double)mem_free / 1e6);
  const int64_t nT = (dn + kInterT - 1) / kInterT;
  NFM_TRY(R->Qc.alloc(sizeof(double) * (size_t)dn * R->Kq));
  NFM_TRY(R->ids.alloc(sizeof(int64_t) * (size_t)dn));
  NFM_TRY(R->sig.alloc(sizeof(uint64_t) * (size_t)dn));
  NFM_TRY(R->tsig.alloc(sizeof(uint64_t) * (size_t)nT));
  hipLaunchKernelGGL(k_inter_rows, dim3(blocks), dim3(kBlock), 0, st, M, order, R->Kq, rowsig.as<uint64_t>(), pos.as<int64_t>(), R->Qc.as<double>(),
                     R->ids.as<int64_t>(), R->sig.as<uint64_t>());
  hipLaunchKernelGGL(k_inter_tsig, dim3((unsigned)std::min<int64_t>((nT + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)ctx->n_cu * 32)), dim3(kBlock), 0, st,
                     dn, nT, R->sig.as<uint64_t>(), R->tsig.as<uint64_t>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // rowsig and pos go back to the block cache: nothing queued may still read them
  return NFM_OK;
}

int inter_stats(nfm_ctx* ctx, const InterRows& R, double* out_l1, int64_t* out_counts) {
  out_l1[0] = out_l1[1] = 0.0;
  out_counts[0] = out_counts[1] = 0;
  out_counts[2] = R.dn;
  if (R.dn == 0) return NFM_OK;
  hipStream_t st = ctx->stream;
  const int64_t nT = (R.dn + kInterT - 1) / kInterT, nTiles = nT * (nT + 1) / 2;
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = (double)nTiles * (2.0 * sizeof(double) + sizeof(uint32_t)) + (double)R.dn * sizeof(int32_t);
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED, "interactionStats: the sums of %lld tiles take %.0f MB and %.0f MB are free", (long long)nTiles,
            bytes / 1e6, (double)mem_free / 1e6);
  DevBuf part, tcount, flags, res;  // res: [res_d[2] | res_c[2]]
  NFM_TRY(part.alloc(sizeof(double) * 2 * (size_t)nTiles));
  NFM_TRY(tcount.alloc(sizeof(uint32_t) * (size_t)nTiles));
  NFM_TRY(flags.alloc(sizeof(int32_t) * (size_t)R.dn));
  NFM_TRY(res.alloc(4 * sizeof(int64_t)));
  NFM_HIP_CHECK(hipMemsetAsync(part.p, 0, sizeof(double) * 2 * (size_t)nTiles, st));
  NFM_HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(int32_t) * (size_t)R.dn, st));
  NFM_HIP_CHECK(hipMemsetAsync(tcount.p, 0, sizeof(uint32_t) * (size_t)nTiles, st));
  double* res_d = res.as<double>();
  int64_t* res_c = res.as<int64_t>() + 2;
  {
    TimedLaunch tl(ctx, "inter_stats");
    const unsigned blocks = (unsigned)std::min<int64_t>(nTiles, (int64_t)ctx->n_cu * kInterGridPerCU);
    hipLaunchKernelGGL(k_inter_stats, dim3(blocks), dim3(kBlock), 0, st, side_of(R), nT, nTiles, R.tsig.as<uint64_t>(), part.as<double>(),
                       tcount.as<uint32_t>(), flags.as<int32_t>());
    hipLaunchKernelGGL(k_inter_fold, dim3(1), dim3(kBlock), 0, st, nTiles, part.as<double>(), R.dn, flags.as<int32_t>(), tcount.as<uint32_t>(), res_d, res_c);
    NFM_HIP_CHECK(hipGetLastError());
  }
  int64_t host[4];
  NFM_HIP_CHECK(hipMemcpyAsync(host, res.p, sizeof(host), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  memcpy(out_l1, host, 2 * sizeof(double));
  out_counts[0] = host[2];
  out_counts[1] = host[3];
  return NFM_OK;
}

int inter_topk(nfm_ctx* ctx, const InterRows& R, int64_t K, int64_t* pairs, double* weights) {
  NFM_CHECK(K >= 1 && K <= kInterMaxTopK, NFM_ERR_INVALID, "topK out of range");
  if (R.dn < 2) {  // no pair
    for (int64_t e = 0; e < K; ++e) {
      pairs[2 * e] = pairs[2 * e + 1] = -1;
      weights[e] = NAN;
    }
    return NFM_OK;
  }
  hipStream_t st = ctx->stream;
  const int64_t nT = (R.dn + kInterT - 1) / kInterT, nTiles = nT * (nT + 1) / 2;
  // the chunk of tiles one workgroup walks; the result does not depend on it
  const int64_t want = std::min<int64_t>(nTiles, (int64_t)ctx->n_cu * kInterGridPerCU);
  const int64_t chunk_tiles = (nTiles + want - 1) / want, chunks = (nTiles + chunk_tiles - 1) / chunk_tiles;
  DevBuf pbits, ppairs, out_p, out_w;
  NFM_TRY(pbits.alloc(sizeof(uint64_t) * (size_t)(chunks * K)));
  NFM_TRY(ppairs.alloc(sizeof(uint64_t) * (size_t)(chunks * K)));
  NFM_TRY(out_p.alloc(sizeof(int64_t) * 2 * (size_t)K));
  NFM_TRY(out_w.alloc(sizeof(double) * (size_t)K));
  {
    TimedLaunch tl(ctx, "inter_topk");
    hipLaunchKernelGGL(k_inter_topk, dim3((unsigned)chunks), dim3(kBlock), (size_t)K * 2 * sizeof(uint64_t), st, side_of(R), nT, nTiles, chunk_tiles,
                       R.tsig.as<uint64_t>(), (int)K, pbits.as<uint64_t>(), ppairs.as<uint64_t>());
    hipLaunchKernelGGL(k_inter_no_pair, dim3(1), dim3(kBlock), 0, st, (int)K, out_p.as<int64_t>(), out_w.as<double>());
    hipLaunchKernelGGL(k_inter_merge, dim3((unsigned)std::min<int64_t>((chunks * K + kBlock - 1) / kBlock, (int64_t)ctx->n_cu * 32)), dim3(kBlock), 0, st,
                       pbits.as<uint64_t>(), ppairs.as<uint64_t>(), chunks, (int)K, R.ids.as<int64_t>(), out_p.as<int64_t>(), out_w.as<double>());
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipMemcpyAsync(pairs, out_p.p, sizeof(int64_t) * 2 * (size_t)K, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipMemcpyAsync(weights, out_w.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

}  // namespace nfm
