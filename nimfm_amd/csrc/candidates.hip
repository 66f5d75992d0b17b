// nimfm_amd/csrc/candidates.hip -- sampleCandidates on the device (candidates.h).
//
//   k_cand_union    per user the ascending distinct union X_i of the rows of exclude and include, the distinct ids of
//                   include's row, and the length of the result's row: one wavefront per user merges 64 ids a round
//   k_cand_sample   per user first(m) as a sorted list in wave-private LDS, then every id of the result's row straight
//                   to its place: one wavefront per user, four users per workgroup
// Integer code throughout (no fp64, no fp32).  No kernel waits for another workgroup, a flag in memory or the host.
#include <algorithm>

#include "candidates.h"

namespace nfm {

namespace {

constexpr int32_t kNoId = 2147483647;        // above every id and every draw
constexpr int kCandSlots = kCandMax / kWave;  // list entries per lane
static_assert(kCandMax % kWave == 0, "a lane holds kCandSlots entries of the list while it is rebuilt");

// what one wavefront has written to LDS is what its lanes read next (cross.hip)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1; }

// the number of entries of a[0, n) below key; a ascends
__device__ __forceinline__ int count_below(const int32_t* a, int n, int32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// elig(r) over X[0, nx), ascending and distinct: X[p] - p does not descend, so the smallest p with X[p] - p > r is found by
// bisection; the p ids below it are the excluded ones that come before the r-th eligible item
__device__ __forceinline__ int32_t elig(const int32_t* __restrict__ X, int nx, int32_t r) {
  int lo = 0, hi = nx;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (X[mid] - mid > r) hi = mid; else lo = mid + 1;
  }
  return r + lo;
}

// ---- the union ----
// A round merges the next 64 ids of the two rows: lane l finds by bisection along its diagonal of the merge path how many
// of the first l merged ids come from exclude's row (an id of exclude goes before an equal one of include), which names its
// own id.  An id equal to its predecessor in the merged order (the lane below; lane 0: the last id of the round before) is
// dropped, the others go to X at the ballot's prefix count.  include's ids that differ from their predecessor in include's
// row go to Bd the same way.  X of user i starts at aptr[i] + bptr[i] and Bd at bptr[i]: room for every id, no scan.
// len[i] = n_i + the distinct ids of include's row; len[nU] = 0 for the scan.
__global__ __launch_bounds__(kBlock) void k_cand_union(int64_t nU, int64_t nV, int64_t n_per, const int64_t* __restrict__ aptr,
                                                       const int32_t* __restrict__ aidx, const int64_t* __restrict__ bptr,
                                                       const int32_t* __restrict__ bidx, int32_t* __restrict__ X, int32_t* __restrict__ Bd,
                                                       int32_t* __restrict__ xlen, int32_t* __restrict__ blen, int64_t* __restrict__ len,
                                                       int* __restrict__ max_row) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  if (blockIdx.x == 0 && threadIdx.x == 0) len[nU] = 0;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nU; u += nwaves) {
    const int64_t a0 = aptr[u], b0 = bptr ? bptr[u] : 0;
    const int64_t la = aptr[u + 1] - a0, lb = bptr ? bptr[u + 1] - b0 : 0;
    const int32_t* A = aidx + a0;
    const int32_t* B = bptr ? bidx + b0 : nullptr;
    int32_t* Xu = X + a0 + b0;
    int32_t* Bu = Bd + b0;
    int64_t ia = 0, ib = 0;  // ids of either row merged so far
    int nx = 0, nb = 0;
    int32_t last = -1;
    while (ia < la || ib < lb) {
      const int64_t ra = la - ia, rb = lb - ib;
      const bool valid = lane < ra + rb;
      int32_t v = kNoId;
      bool from_b = false, b_new = false;
      if (valid) {
        int64_t lo = lane > rb ? lane - rb : 0, hi = lane < ra ? lane : ra;
        while (lo < hi) {  // A[ia + mid] is among the first `lane` ids if it does not exceed B's id on the same diagonal
          const int64_t mid = (lo + hi) >> 1;
          if (A[ia + mid] <= B[ib + lane - 1 - mid]) lo = mid + 1; else hi = mid;
        }
        const int64_t y = lane - lo;  // lo ids of A, y of B come before this lane's
        const int32_t av = lo < ra ? A[ia + lo] : kNoId, bv = y < rb ? B[ib + y] : kNoId;
        from_b = !(lo < ra && (y >= rb || av <= bv));
        v = from_b ? bv : av;
        b_new = from_b && (ib + y == 0 || B[ib + y - 1] != v);
      }
      const int32_t below = __shfl_up(v, 1, kWave);
      const bool keep = valid && v != (lane == 0 ? last : below);
      const unsigned long long mk = __ballot(keep), mb = __ballot(b_new), ma = __ballot(valid && !from_b);
      if (keep) Xu[nx + __popcll(mk & lanes_below(lane))] = v;
      if (b_new) Bu[nb + __popcll(mb & lanes_below(lane))] = v;
      nx += __popcll(mk);
      nb += __popcll(mb);
      const int n_valid = ra + rb < kWave ? (int)(ra + rb) : kWave;
      last = __shfl(v, n_valid - 1, kWave);
      ia += __popcll(ma);
      ib += n_valid - __popcll(ma);
    }
    if (lane == 0) {
      const int64_t E = nV - nx, n = n_per < E ? n_per : E;
      xlen[u] = nx;
      blen[u] = nb;
      len[u] = n + nb;
      atomicMax(max_row, (int)(n + nb));
    }
  }
}

// ---- the sample ----
// lst: the distinct draws so far, ascending, in the wave's own kCandMax int32 of LDS.  A round draws 64 values, lane l draw
// t0 + l: no memory.  A draw is new if it is not in the list (bisection in LDS) and no lower lane of the round carries it
// (a loop of 63 v_readlane: the same cost as a six-step bitonic sort of (value, lane) and nothing to get wrong; a lower lane
// with the same value that is in the list makes no difference, since then this one is too).  The new draws are taken in
// lane order up to the count still missing, so the list never goes past first(m).  Taken draws are distinct and not in the
// list: one's place is the entries below it plus the taken draws below it, an entry moves down by the taken draws below it
// (list_insert's scheme of cross.hip, for up to 64 at once), every lane holding its kCandSlots entries in registers between
// the read and the write.
//
// The row of the result is not merged: every id computes its own place.  With Bu the distinct ids of include's row and
// rank(b) = b - |{x in X_i : x < b}| the eligible items below b:
//   the k-th id s of S_i goes to k + |{b in Bu : b < s}|
//   the q-th id b of Bu goes to q + |{s in S_i : s < b}|, and elig(r) < b exactly when r < rank(b), so that count is
//   c = |{r in lst : r < rank(b)}| in the direct case and rank(b) - c in the complement case
// S_i in the direct case: elig of the list, k the place in the list.  In the complement case the ranks 0 .. E - 1 are walked
// 64 a round against the list with a cursor: the entries at the cursor that fall into the round's window become a 64-bit
// mask, the other ranks are counted by ballot, k = r0 - cursor + the prefix count.
__global__ __launch_bounds__(kBlock) void k_cand_sample(int64_t nU, int64_t nV, int64_t n_per, uint64_t seed, const int64_t* __restrict__ aptr,
                                                        const int64_t* __restrict__ bptr, const int32_t* __restrict__ X,
                                                        const int32_t* __restrict__ Bd, const int32_t* __restrict__ xlen,
                                                        const int32_t* __restrict__ blen, const int64_t* __restrict__ cptr,
                                                        int32_t* __restrict__ cidx) {
  __shared__ int32_t lists[kWavesPerBlock][kCandMax];
  const int lane = threadIdx.x & (kWave - 1);
  int32_t* lst = lists[threadIdx.x >> 6];
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); u < nU; u += nwaves) {
    const int64_t b0 = bptr ? bptr[u] : 0;
    const int32_t* Xu = X + aptr[u] + b0;
    const int32_t* Bu = Bd + b0;
    const int nx = xlen[u], nb = blen[u];
    const int32_t E = (int32_t)(nV - nx);
    const int n = n_per < E ? (int)n_per : E;
    const bool direct = n < E && 2 * (int64_t)n <= E;
    const int m = n == E ? 0 : direct ? n : E - n;  // <= kCandMax: E - n < n in the complement case
    int cnt = 0;
    for (uint64_t t0 = 0; cnt < m; t0 += kWave) {
      const int32_t v = (int32_t)__umul64hi(cand_mix(seed, (uint64_t)u, t0 + lane), (uint64_t)E);
      const int lo = count_below(lst, cnt, v);
      const bool in_list = lo < cnt && lst[lo] == v;
      bool dup = false;
#pragma unroll 8
      for (int s = 0; s < kWave - 1; ++s) dup |= __builtin_amdgcn_readlane(v, s) == v && lane > s;
      const bool fresh = !in_list && !dup;
      const int fresh_below = __popcll(__ballot(fresh) & lanes_below(lane));
      const bool take = fresh && fresh_below < m - cnt;
      const unsigned long long tk = __ballot(take);
      const int slots = (cnt + kWave - 1) / kWave;  // the same for every lane
      int32_t e[kCandSlots];
      int sh[kCandSlots];
#pragma unroll
      for (int c = 0; c < kCandSlots; ++c) {
        sh[c] = 0;
        e[c] = c < slots && lane + c * kWave < cnt ? lst[lane + c * kWave] : kNoId;
      }
      int r = 0;
      for (unsigned long long rest = tk; rest; rest &= rest - 1) {
        const int32_t x = __shfl(v, __ffsll(rest) - 1, kWave);
        r += x < v;
#pragma unroll
        for (int c = 0; c < kCandSlots; ++c)
          if (c < slots) sh[c] += x < e[c];
      }
      wave_lds_fence();  // every lane has read its entries
#pragma unroll
      for (int c = 0; c < kCandSlots; ++c)
        if (c < slots && lane + c * kWave < cnt) lst[lane + c * kWave + sh[c]] = e[c];
      if (take) lst[lo + r] = v;
      cnt += __popcll(tk);
      wave_lds_fence();
    }
    int32_t* out = cidx + cptr[u];
    if (direct) {
      for (int k = lane; k < m; k += kWave) {
        const int32_t s = elig(Xu, nx, lst[k]);
        out[k + count_below(Bu, nb, s)] = s;
      }
    } else {
      int cur = 0;  // list entries below r0
      for (int32_t r0 = 0; r0 < E; r0 += kWave) {  // r0 + kWave <= nV + 63 < 2^31
        const int32_t id = cur + lane < m ? lst[cur + lane] : kNoId;
        const unsigned long long in = __ballot(id < r0 + kWave);  // the list ascends and is distinct: the lanes 0 .. popc - 1
        unsigned long long gone = 0;
        for (unsigned long long rest = in; rest; rest &= rest - 1) gone |= 1ull << (__shfl(id, __ffsll(rest) - 1, kWave) - r0);
        const int32_t r = r0 + lane;
        const bool keep = r < E && !((gone >> lane) & 1);
        const unsigned long long km = __ballot(keep);
        if (keep) {
          const int32_t s = elig(Xu, nx, r);
          out[r0 - cur + __popcll(km & lanes_below(lane)) + count_below(Bu, nb, s)] = s;
        }
        cur += __popcll(in);
      }
    }
    for (int q = lane; q < nb; q += kWave) {
      const int32_t b = Bu[q];
      const int32_t rank = b - count_below(Xu, nx, b);
      const int c = count_below(lst, m, rank);
      out[q + (direct ? c : rank - c)] = b;
    }
    wave_lds_fence();  // the list has been read before the next user's is begun
  }
}

}  // namespace

int sample_candidates(nfm_ctx* ctx, const AscendingRows& exclude, int64_t exclude_nnz, const AscendingRows* include, int64_t include_nnz, int64_t nU,
                      int64_t nV, int64_t n_per_user, uint64_t seed, DsParts* out) {
  hipStream_t st = ctx->stream;
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (size_t)(nU + 1)));
  out->n = nU;
  out->d = nV;
  if (nU == 0) {
    NFM_HIP_CHECK(hipMemsetAsync(out->indptr.p, 0, sizeof(int64_t), st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    return dsop_alloc_entries(out, 0, false);
  }
  DevBuf X, Bd, xlen, blen, len, mx;
  NFM_TRY(X.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(exclude_nnz + include_nnz, 1)));
  NFM_TRY(Bd.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(include_nnz, 1)));
  NFM_TRY(xlen.alloc(sizeof(int32_t) * (size_t)nU));
  NFM_TRY(blen.alloc(sizeof(int32_t) * (size_t)nU));
  NFM_TRY(len.alloc(sizeof(int64_t) * (size_t)(nU + 1)));
  NFM_TRY(mx.alloc(sizeof(int)));
  NFM_HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(int), st));
  const int64_t* bptr = include ? include->indptr : nullptr;
  const int32_t* bidx = include ? include->indices : nullptr;
  // a wavefront per user, grid-strided at what the registers let reside: eight workgroups a CU of the union, five of the sample
  const int64_t groups = (nU + kWavesPerBlock - 1) / kWavesPerBlock;
  const unsigned blocks = (unsigned)std::min<int64_t>(groups, (int64_t)ctx->n_cu * 8);
  {
    TimedLaunch tl(ctx, "cand_union");
    hipLaunchKernelGGL(k_cand_union, dim3(blocks), dim3(kBlock), 0, st, nU, nV, n_per_user, exclude.indptr, exclude.indices, bptr, bidx, X.as<int32_t>(),
                       Bd.as<int32_t>(), xlen.as<int32_t>(), blen.as<int32_t>(), len.as<int64_t>(), mx.as<int>());
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_TRY(dsop_exclusive_scan(st, len.as<int64_t>(), out->indptr.as<int64_t>(), nU + 1));
  int64_t nnz = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&nnz, out->indptr.as<int64_t>() + nU, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipMemcpyAsync(&out->max_row, mx.p, sizeof(int), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  const double bytes = (double)nnz * (sizeof(int32_t) + sizeof(double));
  NFM_CHECK(bytes <= (double)mem_free, NFM_ERR_UNSUPPORTED,
            "sampleCandidates: the result's %lld candidates take %.0f MB and %.0f MB are free: sample row slices of exclude", (long long)nnz, bytes / 1e6,
            (double)mem_free / 1e6);
  NFM_TRY(dsop_alloc_entries(out, nnz, false));
  if (nnz > 0) {
    {
      TimedLaunch tl(ctx, "cand_sample");
      hipLaunchKernelGGL(k_cand_sample, dim3((unsigned)std::min<int64_t>(groups, (int64_t)ctx->n_cu * 5)), dim3(kBlock), 0, st, nU, nV, n_per_user, seed, exclude.indptr, bptr, X.as<int32_t>(), Bd.as<int32_t>(),
                         xlen.as<int32_t>(), blen.as<int32_t>(), out->indptr.as<int64_t>(), out->indices.as<int32_t>());
      NFM_HIP_CHECK(hipGetLastError());
    }
    NFM_TRY(launch_fill(ctx, out->data.as<double>(), nnz, 1.0));
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // the scratch goes back to the block cache: nothing queued may still read it
  return NFM_OK;
}

}  // namespace nfm
