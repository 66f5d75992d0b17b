// nimfm_amd/csrc/dataset_csc.hip -- column-major datasets without leaving HBM.
//
// Replaces, for a dataset resident on the device, the reference's host-side library calls
//   toCSCMatrix / toCSRMatrix     tensor/sparse.nim:510-527 / :490-507 (dataset.nim toCSCDataset, toCSRDataset)
//   X[a..<b] of a CSCMatrix       tensor/sparse.nim:300-330
// Both are copies and integer work: the results are the reference's arrays bit for bit.  No floating-point atomics, no
// kernel that waits for another workgroup.  Launch geometry: dataset_ops.hip's (dsop_grid) -- grid-stride loops over at most
// n_cu * 8 workgroups of 256 threads; 8 lanes per major segment, or a wavefront when the segments average 64 entries or more.
//
// The transposition.  The reference walks the major segments in order and appends each entry to the list of its minor id
// (:516-525): list j ends up holding the entries of id j in ascending storage position.  That IS a stable sort of the
// storage positions by minor id, so:
//   1. every entry's major id, written by a lane group per segment (no search per entry: dataset_ops.hip measured that);
//   2. a stable radix sort (hipcub) of (minor id, storage position) over the bits the minor dimension needs;
//   3. the new pointer from integer counts per minor id (integer atomics) and an int64 exclusive scan;
//   4. a gather of major ids and values through the sorted positions.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "dataset_csc.h"

namespace nfm {
namespace {

constexpr int kG = 8;  // lanes per major segment

#define CSC_LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__)

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

// major[q] = the segment entry q lies in; pos[q] = q
template <int G>
__global__ __launch_bounds__(kBlock) void k_major_ids(int64_t n, const int64_t* __restrict__ ptr, int32_t* __restrict__ major,
                                                      int32_t* __restrict__ pos) {
  const int gl = threadIdx.x & (G - 1);
  for (int64_t s = gtid() / G; s < n; s += gstride() / G) {
    const int64_t q1 = ptr[s + 1];
    for (int64_t q = ptr[s] + gl; q < q1; q += G) {
      major[q] = (int32_t)s;
      pos[q] = (int32_t)q;
    }
  }
}

// cnt[j] += 1 per entry of minor id j (cnt is zeroed, d + 1 long: the scan's closing element stays 0)
__global__ __launch_bounds__(kBlock) void k_count_minor(int64_t nnz, const int32_t* __restrict__ idx, unsigned long long* __restrict__ cnt) {
  for (int64_t q = gtid(); q < nnz; q += gstride()) atomicAdd(&cnt[idx[q]], 1ull);
}

__global__ __launch_bounds__(kBlock) void k_gather(int64_t nnz, const int32_t* __restrict__ spos, const int32_t* __restrict__ major,
                                                   const double* __restrict__ val, int32_t* __restrict__ out_idx,
                                                   double* __restrict__ out_val) {
  for (int64_t c = gtid(); c < nnz; c += gstride()) {
    const int32_t p = spos[c];
    out_idx[c] = major[p];
    out_val[c] = val[p];
  }
}

// the longest of the d segments of ptr
__global__ __launch_bounds__(kBlock) void k_max_len(int64_t d, const int64_t* __restrict__ ptr, int* __restrict__ max_len) {
  int mx = 0;
  for (int64_t j = gtid(); j < d; j += gstride()) {
    const int64_t l = ptr[j + 1] - ptr[j];
    mx = l > mx ? (int)(l > 2147483647 ? 2147483647 : l) : mx;
  }
  for (int s = 1; s < kWave; s <<= 1) {
    const int o = __shfl_xor(mx, s, kWave);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && mx > 0) atomicMax(max_len, mx);
}

// ---- the row range of a column-major dataset ----
// len[s] = entries of segment s with begin <= id < end; len[n] = 0 for the scan
template <int G>
__global__ __launch_bounds__(kBlock) void k_filter_count(int64_t n, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                         int64_t begin, int64_t end, int64_t* __restrict__ len) {
  const int gl = threadIdx.x & (G - 1);
  if (gtid() == 0) len[n] = 0;
  for (int64_t s = gtid() / G; s < n; s += gstride() / G) {
    const int64_t q1 = ptr[s + 1];
    int c = 0;
    for (int64_t q = ptr[s] + gl; q < q1; q += G) {
      const int64_t i = idx[q];
      c += (i >= begin && i < end) ? 1 : 0;
    }
    for (int w = 1; w < G; w <<= 1) c += __shfl_xor(c, w, G);
    if (gl == 0) len[s] = c;
  }
}

// G entries of a segment at a time: the kept ones land behind the segment's earlier kept entries in their own order -- a
// ballot of the group's lanes and the count of kept lanes below one's own
template <int G>
__global__ __launch_bounds__(kBlock) void k_filter_fill(int64_t n, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                        const double* __restrict__ val, int64_t begin, int64_t end,
                                                        const int64_t* __restrict__ out_ptr, int32_t* __restrict__ out_idx,
                                                        double* __restrict__ out_val) {
  const int gl = threadIdx.x & (G - 1), base = (threadIdx.x & (kWave - 1)) & ~(G - 1);
  const unsigned long long gmask = G == kWave ? ~0ull : ((1ull << (G & 63)) - 1ull);
  for (int64_t s = gtid() / G; s < n; s += gstride() / G) {
    const int64_t q0 = ptr[s], q1 = ptr[s + 1];
    int64_t dst = out_ptr[s];
    if (out_ptr[s + 1] == dst) continue;  // nothing of this segment is kept
    for (int64_t c = q0; c < q1; c += G) {
      const int64_t q = c + gl;
      const int64_t i = q < q1 ? (int64_t)idx[q] : -1;
      const bool keep = q < q1 && i >= begin && i < end;
      const unsigned long long grp = (__ballot(keep) >> base) & gmask;
      if (keep) {
        const int64_t o = dst + __popcll(grp & ((1ull << gl) - 1ull));
        out_idx[o] = (int32_t)(i - begin);
        out_val[o] = val[q];
      }
      dst += __popcll(grp);
    }
  }
}

}  // namespace

int dsop_transpose(nfm_ctx* ctx, const CsrView& X, DsParts* out) {
  hipStream_t st = ctx->stream;
  const int64_t n = X.n, d = X.d, nnz = X.nnz;
  NFM_CHECK(nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a transposition of more than 2^31-2 entries");
  NFM_CHECK(n <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "%lld rows / columns do not fit the int32 ids of the other layout", (long long)n);
  DevBuf major, pos, spos, skey, cnt, mx, tmp;
  NFM_TRY(cnt.alloc(sizeof(int64_t) * (d + 1)));
  NFM_TRY(mx.alloc(sizeof(int)));
  NFM_HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int64_t) * (d + 1), st));
  NFM_HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(int), st));
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (d + 1)));
  NFM_TRY(dsop_alloc_entries(out, nnz, false));
  if (nnz) {
    NFM_TRY(major.alloc(sizeof(int32_t) * nnz));
    NFM_TRY(pos.alloc(sizeof(int32_t) * nnz));
    NFM_TRY(spos.alloc(sizeof(int32_t) * nnz));
    NFM_TRY(skey.alloc(sizeof(int32_t) * nnz));
    if (nnz / n >= kWave)
      CSC_LAUNCH(k_major_ids<kWave>, dsop_grid(ctx, n, kBlock / kWave), n, X.indptr, major.as<int32_t>(), pos.as<int32_t>());
    else
      CSC_LAUNCH(k_major_ids<kG>, dsop_grid(ctx, n, kBlock / kG), n, X.indptr, major.as<int32_t>(), pos.as<int32_t>());
    CSC_LAUNCH(k_count_minor, dsop_grid(ctx, nnz), nnz, X.indices, cnt.as<unsigned long long>());
    NFM_HIP_CHECK(hipGetLastError());
    int end_bit = 1;
    while (end_bit < 31 && ((int64_t)1 << end_bit) < d) ++end_bit;
    size_t bytes = 0;
    NFM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, X.indices, skey.as<int32_t>(), pos.as<int32_t>(), spos.as<int32_t>(),
                                                     (int)nnz, 0, end_bit, st));
    NFM_TRY(tmp.alloc(bytes));
    NFM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, X.indices, skey.as<int32_t>(), pos.as<int32_t>(), spos.as<int32_t>(),
                                                     (int)nnz, 0, end_bit, st));
    CSC_LAUNCH(k_gather, dsop_grid(ctx, nnz), nnz, spos.as<int32_t>(), major.as<int32_t>(), X.data, out->indices.as<int32_t>(),
               out->data.as<double>());
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_TRY(dsop_exclusive_scan(st, cnt.as<int64_t>(), out->indptr.as<int64_t>(), d + 1));
  if (d) CSC_LAUNCH(k_max_len, dsop_grid(ctx, d), d, out->indptr.as<int64_t>(), mx.as<int>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_HIP_CHECK(hipMemcpyAsync(&out->max_row, mx.p, sizeof(int), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // the scratch goes back to the block cache on return
  out->n = d;
  out->d = n;
  out->n_fields = 0;
  return NFM_OK;
}

int dsop_filter_minor(nfm_ctx* ctx, const CsrView& X, int64_t begin, int64_t end, DsParts* out) {
  hipStream_t st = ctx->stream;
  const int64_t n = X.n;
  const bool wave = n > 0 && X.nnz / n >= kWave;
  DevBuf len;
  NFM_TRY(len.alloc(sizeof(int64_t) * (n + 1)));
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (n + 1)));
  if (wave)
    CSC_LAUNCH(k_filter_count<kWave>, dsop_grid(ctx, n, kBlock / kWave), n, X.indptr, X.indices, begin, end, len.as<int64_t>());
  else
    CSC_LAUNCH(k_filter_count<kG>, dsop_grid(ctx, n, kBlock / kG), n, X.indptr, X.indices, begin, end, len.as<int64_t>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(dsop_exclusive_scan(st, len.as<int64_t>(), out->indptr.as<int64_t>(), n + 1));
  int64_t nnz = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&nnz, out->indptr.as<int64_t>() + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  NFM_TRY(dsop_alloc_entries(out, nnz, false));
  if (nnz) {
    if (wave)
      CSC_LAUNCH(k_filter_fill<kWave>, dsop_grid(ctx, n, kBlock / kWave), n, X.indptr, X.indices, X.data, begin, end, out->indptr.as<int64_t>(),
                 out->indices.as<int32_t>(), out->data.as<double>());
    else
      CSC_LAUNCH(k_filter_fill<kG>, dsop_grid(ctx, n, kBlock / kG), n, X.indptr, X.indices, X.data, begin, end, out->indptr.as<int64_t>(),
                 out->indices.as<int32_t>(), out->data.as<double>());
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // len goes back to the block cache on return
  out->n = n;
  out->d = end - begin;
  out->n_fields = 0;
  out->max_row = 0;
  return NFM_OK;
}

}  // namespace nfm
