// nimfm_amd/csrc/extmath.hip -- sparse x dense products of resident datasets (extmath.h).
//
// The reference's loops (extmath.nim:10-133) add `a * b` to one output element at a time, in an order the matrix's storage
// fixes; the library is built with -ffp-contract=off.  Every output element here is ONE chain `acc = acc + (val * D[j][c])`
// from +0.0 over the entries of its segment in storage order, held in one register of one lane from the first entry to the
// last: the reference's bits.
//   k_spmm<T, A, VEC>   a team of T lanes owns a segment (a row of S, or a column of S through the transposed view); lane t owns
//                       the 16-byte words t, t + T, ... of the dense row, A of them per column panel, each a double2 accumulator.
//                       The (id, value) pairs of all segments of a wavefront are one contiguous range of the entry arrays: the
//                       wavefront reads it into LDS in coalesced 16-byte words, kSpmmStage entries at a time, and the teams read
//                       their entries from there (a broadcast inside a team).  kSpmmUnroll dense rows are in flight per lane; the
//                       adds are retired in entry order.
//   k_transpose_f64     a dense matrix transposed through padded 32 x 32 tiles in LDS: D . S is (S^T . D^T)^T
// No kernel waits for another workgroup, a flag in memory or the host, and there is no atomic operation: the bits of an output
// element depend on its segment and the dense operand alone.
#include <algorithm>

#include "extmath.h"

namespace nfm {

namespace {

constexpr int kStageLd = kSpmmStage + kSpmmStage / 32;  // one slot of padding per 32 entries: 64 rows of 32 entries at T = 1
                                                        // would otherwise start in two LDS banks
static_assert(kSpmmStage == 4 * kWave, "a lane stages four entries: one 16-byte word of ids, two of values");

// what one wavefront has written to LDS is what its lanes read next (and the reverse, before the buffer is refilled)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int stage_slot(int p) { return p + (p >> 5); }

// word w of a dense row of r doubles (W words, the last one half full when r is odd); zero beyond the row
template <bool VEC>
__device__ __forceinline__ double2 load_word(const double* __restrict__ row, int w, int W, int r) {
  double2 v = make_double2(0.0, 0.0);
  if (VEC) {
    if (w < W) v = *reinterpret_cast<const double2*>(row + 2 * w);
  } else {
    const int c = 2 * w;
    if (c < r) v.x = row[c];
    if (c + 1 < r) v.y = row[c + 1];
  }
  return v;
}

// VEC: r is even and D, R are 16-byte aligned, so a word is one 16-byte access; otherwise its doubles are read and written one
// by one (the same values: the layout of the access is no part of a chain).  ent_vec: the entry arrays are 16-byte aligned.
template <int T, int A, bool VEC>
__global__ __launch_bounds__(kBlock) void k_spmm(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                 const double* __restrict__ data, int64_t nnz, int ent_vec, const double* __restrict__ D, int r,
                                                 double* __restrict__ R) {
  constexpr int RPW = kWave / T, U = kSpmmUnroll;
  __shared__ int32_t s_idx[kWavesPerBlock][kStageLd];
  __shared__ double s_val[kWavesPerBlock][kStageLd];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int team = lane / T, t = lane % T;
  const int W = (r + 1) >> 1;
  int32_t* sidx = s_idx[wv];
  double* sval = s_val[wv];
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + wv, nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t i0 = wave0 * RPW; i0 < n; i0 += nwaves * RPW) {
    const int64_t i = i0 + team;
    const bool valid = i < n;
    const int64_t q0 = valid ? indptr[i] : 0, q1 = valid ? indptr[i + 1] : 0;
    const int64_t e0 = indptr[i0], e1 = indptr[i0 + RPW < n ? i0 + RPW : n];  // the entries of the wavefront's segments
    for (int w0 = 0; w0 < W; w0 += T * A) {  // one column panel: a fresh pass over the entries
      double2 acc[A];
#pragma unroll
      for (int a = 0; a < A; ++a) acc[a] = make_double2(0.0, 0.0);
      for (int64_t b = e0 & ~(int64_t)3; b < e1; b += kSpmmStage) {
        wave_lds_fence();  // the teams are done with the entries staged before
        {
          const int64_t g = b + 4 * lane;
          int32_t j4[4];
          double v4[4];
          if (ent_vec && g + 3 < nnz) {
            const int4 jj = *reinterpret_cast<const int4*>(indices + g);
            const double2 va = *reinterpret_cast<const double2*>(data + g), vb = *reinterpret_cast<const double2*>(data + g + 2);
            j4[0] = jj.x; j4[1] = jj.y; j4[2] = jj.z; j4[3] = jj.w;
            v4[0] = va.x; v4[1] = va.y; v4[2] = vb.x; v4[3] = vb.y;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const bool in = g + k < nnz;
              j4[k] = in ? indices[g + k] : 0;
              v4[k] = in ? data[g + k] : 0.0;
            }
          }
          const int s = stage_slot(4 * lane);  // the four slots of a lane lie inside one run of 32
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            sidx[s + k] = j4[k];
            sval[s + k] = v4[k];
          }
        }
        wave_lds_fence();
        const int64_t lo = q0 > b ? q0 : b, hi = q1 < b + kSpmmStage ? q1 : b + kSpmmStage;
        int p = (int)(lo - b);
        const int pe = hi > lo ? (int)(hi - b) : p;
        for (; p + U <= pe; p += U) {
          double x[U];
          double2 dv[U][A];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int s = stage_slot(p + u);
            const double* row = D + (size_t)sidx[s] * (size_t)r;
            x[u] = sval[s];
#pragma unroll
            for (int a = 0; a < A; ++a) dv[u][a] = load_word<VEC>(row, w0 + t + a * T, W, r);
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int a = 0; a < A; ++a) {
              acc[a].x = acc[a].x + x[u] * dv[u][a].x;
              acc[a].y = acc[a].y + x[u] * dv[u][a].y;
            }
        }
        for (; p < pe; ++p) {
          const int s = stage_slot(p);
          const double* row = D + (size_t)sidx[s] * (size_t)r;
          const double x = sval[s];
          double2 dv[A];
#pragma unroll
          for (int a = 0; a < A; ++a) dv[a] = load_word<VEC>(row, w0 + t + a * T, W, r);
#pragma unroll
          for (int a = 0; a < A; ++a) {
            acc[a].x = acc[a].x + x * dv[a].x;
            acc[a].y = acc[a].y + x * dv[a].y;
          }
        }
      }
      if (valid) {
        double* out = R + (size_t)i * (size_t)r;
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const int w = w0 + t + a * T;
          if (VEC) {
            if (w < W) *reinterpret_cast<double2*>(out + 2 * w) = acc[a];
          } else {
            if (2 * w < r) out[2 * w] = acc[a].x;
            if (2 * w + 1 < r) out[2 * w + 1] = acc[a].y;
          }
        }
      }
    }
  }
}

template <int T, int A>
int launch_spmm_TA(nfm_ctx* ctx, const CsrView& X, const double* D, int r, double* R) {
  constexpr int RPW = kWave / T;
  const int64_t per_block = (int64_t)kWavesPerBlock * RPW;
  int64_t blocks = (X.n + per_block - 1) / per_block;
  const int64_t cap = (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 32;
  if (blocks > cap) blocks = cap;
  const bool vec = r % 2 == 0 && (reinterpret_cast<uintptr_t>(D) & 15) == 0 && (reinterpret_cast<uintptr_t>(R) & 15) == 0;
  const int ent_vec = (reinterpret_cast<uintptr_t>(X.indices) & 15) == 0 && (reinterpret_cast<uintptr_t>(X.data) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((k_spmm<T, A, true>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, X.n, X.indptr, X.indices, X.data, X.nnz, ent_vec,
                       D, r, R);
  else
    hipLaunchKernelGGL((k_spmm<T, A, false>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, X.n, X.indptr, X.indices, X.data, X.nnz, ent_vec,
                       D, r, R);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

constexpr int kTile = 32;
static_assert(kBlock == kTile * 8, "a workgroup moves a tile in four trips of eight rows");

// tile[k][tx] is written by rows and read by columns: 33 doubles per row put the 32 doubles of a column into 32 different
// 8-byte bank pairs
__global__ __launch_bounds__(kBlock) void k_transpose_f64(const double* __restrict__ in, int64_t rows, int64_t cols, double* __restrict__ out) {
  __shared__ double tile[kTile][kTile + 1];
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
  const int64_t tc = (cols + kTile - 1) / kTile, tiles = tc * ((rows + kTile - 1) / kTile);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {  // (the trip count is the workgroup's: the barriers are uniform)
    const int64_t r0 = ti / tc * kTile, c0 = ti % tc * kTile;
    for (int k = ty; k < kTile; k += kBlock / kTile)
      if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = in[(size_t)(r0 + k) * (size_t)cols + (size_t)(c0 + tx)];
    __syncthreads();
    for (int k = ty; k < kTile; k += kBlock / kTile)
      if (c0 + k < cols && r0 + tx < rows) out[(size_t)(c0 + k) * (size_t)rows + (size_t)(r0 + tx)] = tile[tx][k];
    __syncthreads();
  }
}

}  // namespace

int launch_spmm(nfm_ctx* ctx, const CsrView& X, const double* D, int64_t r, double* R) {
  NFM_CHECK(r >= 0 && r < ((int64_t)1 << 30), NFM_ERR_UNSUPPORTED, "a dense operand of %lld columns", (long long)r);
  if (X.n == 0 || r == 0) return NFM_OK;
  TimedLaunch tl(ctx, "extmath_spmm");
  const int T = spmm_team(r);
  const int64_t per_lane = ((r + 1) / 2 + T - 1) / T;  // 16-byte words a lane owns
  if (per_lane <= 1) return with_lanes(T, [&](auto L) { return launch_spmm_TA<L(), 1>(ctx, X, D, (int)r, R); });
  if (per_lane <= 2) return launch_spmm_TA<kWave, 2>(ctx, X, D, (int)r, R);
  return launch_spmm_TA<kWave, kSpmmAcc>(ctx, X, D, (int)r, R);
}

int launch_transpose_f64(nfm_ctx* ctx, const double* in, int64_t rows, int64_t cols, double* out) {
  if (rows == 0 || cols == 0) return NFM_OK;
  TimedLaunch tl(ctx, "extmath_transpose");
  const int64_t tiles = ((rows + kTile - 1) / kTile) * ((cols + kTile - 1) / kTile);
  const int64_t cap = (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 32;
  hipLaunchKernelGGL(k_transpose_f64, dim3((unsigned)std::min(tiles, cap)), dim3(kBlock), 0, ctx->stream, in, rows, cols, out);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

}  // namespace nfm
