// nimfm_amd/csrc/dataset_ops.hip -- datasets made from datasets without leaving HBM.
//
// Replaces, for a dataset resident on the device, the reference's host-side library calls
//   X[indices], X[a..<b]          tensor/sparse.nim:263-285, 333-357 (dataset.nim:319-369)
//   vstack / hstack               tensor/sparse.nim:564-581, 613-633 / :671-698, 719-750
//   normalize(X, axis, norm)      tensor/sparse.nim:372-411 (dataset.nim:398-403)
//   loadUserItemRatingFile        dataset.nim:840-900
// Every result is a NEW set of arrays; the inputs are only read.  All work is issued on the context's stream: row lengths,
// an int64 exclusive scan (hipcub), one small read-back of the sizes, copy kernels that write contiguously (no runtime
// device-to-device copies: a plain copy is a kernel too).  No
// floating-point atomics anywhere: a norm is a fold over the entries in the reference's order (8 lanes per row / column,
// 8 entries at a time, combined lane by lane through shuffles -- cfm_dev.h's ordered_acc with the norm's own step), so the
// results are the reference's bits.
//
// Launch geometry: every kernel walks its work in a grid-stride loop over at most n_cu * 8 workgroups of 256 threads
// (32 wavefronts per CU: full occupancy for kernels that only move bytes) -- 524288 elements per pass of an element-wise
// kernel, 65536 rows / columns per pass of a kernel with 8 lanes per row, 8192 per pass of one with a wavefront per row, on 256 CUs.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "dataset_ops.h"
#include "ingest.h"
#include "parse_num.h"

namespace nfm {
namespace {

constexpr int kG = 8;                 // lanes per row / column
constexpr int kGroups = kBlock / kG;  // rows / columns per workgroup

#define DS_LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__)

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

__device__ __forceinline__ void wave_max_to(int v, int* dst) {
  for (int s = 1; s < kWave; s <<= 1) {
    const int o = __shfl_xor(v, s, kWave);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && v > 0) atomicMax(dst, v);
}

// ---- row selection ---------------------------------------------------------------------------------------------------
// len[ii] = length of input row rows[ii] (rows == nullptr: begin + ii), len[m] = 0 for the scan; the target follows
__global__ __launch_bounds__(kBlock) void k_sel_len(int64_t m, const int64_t* __restrict__ rows, int64_t begin,
                                                    const int64_t* __restrict__ in_ptr, const double* __restrict__ in_y,
                                                    int64_t* __restrict__ len, double* __restrict__ out_y, int* __restrict__ max_row) {
  int mx = 0;
  for (int64_t ii = gtid(); ii <= m; ii += gstride()) {
    if (ii == m) {
      len[ii] = 0;
    } else {
      const int64_t r = rows ? rows[ii] : begin + ii;
      const int64_t l = in_ptr[r + 1] - in_ptr[r];
      len[ii] = l;
      if (in_y) out_y[ii] = in_y[r];
      mx = l > mx ? (int)l : mx;
    }
  }
  wave_max_to(mx, max_row);
}

// G lanes per OUTPUT row (8, or a wavefront when the rows average 64 entries or more): one look at the two indptrs per row,
// then the row's entries G at a time.  Writes are contiguous: a row's entries follow the previous row's.
// (One thread per output entry finding its row by binary search over the new indptr -- what ingest.hip does per entry --
// was measured first: 2.5e9 entries/s on cfg2's shape, the ~20 dependent reads per entry being the whole cost; DESIGN.md
// section 23.)
template <int G>
__global__ __launch_bounds__(kBlock) void k_sel_rows(int64_t m, const int64_t* __restrict__ out_ptr, const int64_t* __restrict__ rows,
                                                     const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_idx,
                                                     const double* __restrict__ in_val, const int32_t* __restrict__ in_fld,
                                                     int32_t* __restrict__ out_idx, double* __restrict__ out_val,
                                                     int32_t* __restrict__ out_fld) {
  const int gl = threadIdx.x & (G - 1);
  for (int64_t ii = gtid() / G; ii < m; ii += gstride() / G) {
    const int64_t dst = out_ptr[ii], len = out_ptr[ii + 1] - dst, src = in_ptr[rows[ii]];
    for (int64_t e = gl; e < len; e += G) {
      out_idx[dst + e] = in_idx[src + e];
      out_val[dst + e] = in_val[src + e];
      if (in_fld) out_fld[dst + e] = in_fld[src + e];
    }
  }
}

// dst[0, n) = src[0, n) in words of T
template <class T>
__global__ __launch_bounds__(kBlock) void k_copy(int64_t n, const T* __restrict__ src, T* __restrict__ dst) {
  for (int64_t i = gtid(); i < n; i += gstride()) dst[i] = src[i];
}

// ---- vstack ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_shift_ptr(int64_t n, const int64_t* __restrict__ in_ptr, int64_t shift,
                                                      int64_t* __restrict__ out_ptr) {
  for (int64_t i = gtid(); i <= n; i += gstride()) out_ptr[i] = in_ptr[i] + shift;
}

// ---- hstack ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_hs_len(int64_t n, const int64_t* __restrict__ part_ptr, int64_t* __restrict__ len, int first,
                                                   int last, int* __restrict__ max_row) {
  int mx = 0;
  for (int64_t i = gtid(); i <= n; i += gstride()) {
    if (i == n) {
      len[i] = 0;
    } else {
      const int64_t l = (first ? 0 : len[i]) + (part_ptr[i + 1] - part_ptr[i]);
      len[i] = l;
      if (last) mx = l > mx ? (int)(l > 2147483647 ? 2147483647 : l) : mx;
    }
  }
  wave_max_to(mx, max_row);
}

// G lanes per row of ONE part: the part's row lands at the row's cursor (where the earlier parts' entries of the row end)
template <int G>
__global__ __launch_bounds__(kBlock) void k_hs_rows(int64_t n, const int64_t* __restrict__ part_ptr, const int32_t* __restrict__ idx,
                                                    const double* __restrict__ val, const int32_t* __restrict__ fld,
                                                    const int64_t* __restrict__ cur, int32_t col_off, int32_t fld_off,
                                                    int32_t* __restrict__ out_idx, double* __restrict__ out_val,
                                                    int32_t* __restrict__ out_fld) {
  const int gl = threadIdx.x & (G - 1);
  for (int64_t i = gtid() / G; i < n; i += gstride() / G) {
    const int64_t src = part_ptr[i], len = part_ptr[i + 1] - src, dst = cur[i];
    for (int64_t e = gl; e < len; e += G) {
      out_idx[dst + e] = idx[src + e] + col_off;
      out_val[dst + e] = val[src + e];
      if (fld) out_fld[dst + e] = fld[src + e] + fld_off;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_hs_advance(int64_t n, const int64_t* __restrict__ part_ptr, int64_t* __restrict__ cur) {
  for (int64_t i = gtid(); i < n; i += gstride()) cur[i] += part_ptr[i + 1] - part_ptr[i];
}

// ---- normalize -------------------------------------------------------------------------------------------------------
// the reference's incremental update f (tensor/sparse.nim:405-411); Nim's max(x, y) is `if y <= x: x else: y`
template <int NORM>
__device__ __forceinline__ double norm_step(double acc, double v) {
  if (NORM == NORM_L2) return acc + v * v;
  const double a = fabs(v);
  if (NORM == NORM_L1) return acc + a;
  return a <= acc ? acc : a;
}

// f(... f(f(0, val(q0)), val(q0 + 1)) ..., val(q1 - 1)), then g; the kG lanes of a group call it together and all return
// the same value.  `base` is the group's first lane in the wavefront.
template <int NORM, class F>
__device__ __forceinline__ double ordered_norm(int64_t q0, int64_t q1, int gl, int base, F val) {
  double acc = 0.0;
  for (int64_t c = q0; c < q1; c += kG) {
    const int64_t q = c + gl;
    const double t = q < q1 ? val(q) : 0.0;
#pragma unroll
    for (int u = 0; u < kG; ++u) {
      const double tu = __shfl(t, base + u, kWave);
      if (c + u < q1) acc = norm_step<NORM>(acc, tu);
    }
  }
  return NORM == NORM_L2 ? __dsqrt_rn(acc) : acc;
}

template <int NORM>
__global__ __launch_bounds__(kBlock) void k_norm_rows(int64_t n, const int64_t* __restrict__ ptr, const double* __restrict__ val,
                                                      double* __restrict__ out) {
  const int gl = threadIdx.x & (kG - 1), base = (threadIdx.x & (kWave - 1)) & ~(kG - 1);
  for (int64_t r = gtid() / kG; r < n; r += gstride() / kG) {
    const int64_t q0 = ptr[r], q1 = ptr[r + 1];
    const double nv = ordered_norm<NORM>(q0, q1, gl, base, [&](int64_t q) { return val[q]; });
    for (int64_t q = q0 + gl; q < q1; q += kG) out[q] = nv != 0.0 ? val[q] / nv : val[q];
  }
}

__global__ __launch_bounds__(kBlock) void k_iota32(int64_t n, int32_t* __restrict__ p) {
  for (int64_t i = gtid(); i < n; i += gstride()) p[i] = (int32_t)i;
}

// cptr[j] = number of entries with a column id below j, from the ids in ascending order
__global__ __launch_bounds__(kBlock) void k_col_ptr(int64_t d, const int32_t* __restrict__ keys, int64_t nnz, int64_t* __restrict__ cptr) {
  for (int64_t j = gtid(); j <= d; j += gstride()) {
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)keys[mid] < j) lo = mid + 1; else hi = mid;
    }
    cptr[j] = lo;
  }
}

// a column's entries in ascending storage position (spos: the stable sort of the positions by column id)
template <int NORM>
__global__ __launch_bounds__(kBlock) void k_norm_cols(int64_t d, const int64_t* __restrict__ cptr, const int32_t* __restrict__ spos,
                                                      const double* __restrict__ val, double* __restrict__ norms) {
  const int gl = threadIdx.x & (kG - 1), base = (threadIdx.x & (kWave - 1)) & ~(kG - 1);
  for (int64_t j = gtid() / kG; j < d; j += gstride() / kG) {
    const double nv = ordered_norm<NORM>(cptr[j], cptr[j + 1], gl, base, [&](int64_t c) { return val[spos[c]]; });
    if (gl == 0) norms[j] = nv;
  }
}

__global__ __launch_bounds__(kBlock) void k_div_cols(int64_t nnz, const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                     const double* __restrict__ norms, double* __restrict__ out) {
  for (int64_t q = gtid(); q < nnz; q += gstride()) {
    const double nv = norms[idx[q]];
    out[q] = nv != 0.0 ? val[q] / nv : val[q];
  }
}

// ---- user item rating ------------------------------------------------------------------------------------------------
enum { UI_BAD = 0, UI_FIRST_BAD = 1, UI_MIN_USER = 2, UI_MAX_USER = 3, UI_MIN_ITEM = 4, UI_MAX_ITEM = 5, UI_LONG = 6, UI_COUNT = 8 };

__device__ __forceinline__ int64_t skip_to_digit(const char* __restrict__ t, int64_t p, int64_t e) {
  while (p < e && !num::is_digit(t[p])) ++p;
  return p;
}

// one thread per line (dataset.nim:871-887)
__global__ __launch_bounds__(kBlock) void k_ui_lines(const char* __restrict__ t, int64_t len, const int64_t* __restrict__ nl, int64_t n_nl,
                                                     int64_t n_lines, const num::Pow5* __restrict__ table, int64_t* __restrict__ keep,
                                                     int64_t* __restrict__ user, int64_t* __restrict__ item, double* __restrict__ rating,
                                                     long long* __restrict__ st, int min_len) {
  long long mnu = INT64_MAX, mxu = INT64_MIN, mni = INT64_MAX, mxi = INT64_MIN;
  for (int64_t i = gtid(); i <= n_lines; i += gstride()) {
    if (i == n_lines) {
      keep[i] = 0;
      continue;
    }
    const int64_t s = i ? nl[i - 1] + 1 : 0;
    int64_t e = i < n_nl ? nl[i] : len;
    if (e > s && t[e - 1] == '\r') --e;
    int64_t k = 0;
    // shorter lines are skipped by every pass: fewer than 4 characters (:853, :872), or fewer than 5 for the loader of a
    // column-major dataset (:923, :955, :975), which therefore never meets the four-character line the next test is about
    if (e - s >= min_len) {
      int64_t u = 0, it = 0;
      double v = 0.0;
      int fl = 0;
      bool ok = e - s > 4;  // exactly four characters: counted by the first pass, skipped by the second
      int64_t p = s;
      if (ok) {
        p = skip_to_digit(t, p, e);
        const int c = p < e ? num::parse_int(t + p, e - p, &u) : 0;
        ok = c > 0 && c <= 18;
        p += c;
      }
      if (ok) {
        p = skip_to_digit(t, p, e);
        const int c = p < e ? num::parse_int(t + p, e - p, &it) : 0;
        ok = c > 0 && c <= 18;
        p += c;
      }
      if (ok) {
        p = skip_to_digit(t, p, e);
        ok = p < e && num::parse_float(t + p, e - p, &v, &fl, table) > 0;
      }
      if (ok) {
        k = 1;
        user[i] = u;
        item[i] = it;
        rating[i] = v;
        mnu = u < mnu ? u : mnu;
        mxu = u > mxu ? u : mxu;
        mni = it < mni ? it : mni;
        mxi = it > mxi ? it : mxi;
        if (fl & num::kNeedsStrtod) atomicAdd((unsigned long long*)&st[UI_LONG], 1ull);
      } else {
        atomicAdd((unsigned long long*)&st[UI_BAD], 1ull);
        atomicMin(&st[UI_FIRST_BAD], (long long)i);
      }
    }
    keep[i] = k;
  }
  for (int s = 1; s < kWave; s <<= 1) {
    const long long a = __shfl_xor(mnu, s, kWave), b = __shfl_xor(mxu, s, kWave);
    const long long c = __shfl_xor(mni, s, kWave), d = __shfl_xor(mxi, s, kWave);
    mnu = a < mnu ? a : mnu;
    mxu = b > mxu ? b : mxu;
    mni = c < mni ? c : mni;
    mxi = d > mxi ? d : mxi;
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && mnu != INT64_MAX) {
    atomicMin(&st[UI_MIN_USER], mnu);
    atomicMax(&st[UI_MAX_USER], mxu);
    atomicMin(&st[UI_MIN_ITEM], mni);
    atomicMax(&st[UI_MAX_ITEM], mxi);
  }
}

// row r = rowof[i] of every kept line: {user - minUser: 1, nUsers + item - minItem: 1} (dataset.nim:896-898)
__global__ __launch_bounds__(kBlock) void k_ui_fill(int64_t n_lines, int64_t n_rows, const int64_t* __restrict__ keep,
                                                    const int64_t* __restrict__ rowof, const int64_t* __restrict__ user,
                                                    const int64_t* __restrict__ item, const double* __restrict__ rating, int64_t min_user,
                                                    int64_t item_shift, int64_t* __restrict__ ptr, int32_t* __restrict__ idx,
                                                    double* __restrict__ val, double* __restrict__ y) {
  for (int64_t i = gtid(); i <= n_lines; i += gstride()) {
    if (i == n_lines) {
      ptr[n_rows] = 2 * n_rows;
    } else if (keep[i]) {
      const int64_t r = rowof[i];
      ptr[r] = 2 * r;
      idx[2 * r] = (int32_t)(user[i] - min_user);
      idx[2 * r + 1] = (int32_t)(item[i] + item_shift);
      val[2 * r] = 1.0;
      val[2 * r + 1] = 1.0;
      y[r] = rating[i];
    }
  }
}

}  // namespace

int dsop_exclusive_scan(hipStream_t st, const int64_t* in, int64_t* out, int64_t count) {
  NFM_CHECK(count < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "more than 2^31-2 rows");
  size_t bytes = 0;
  DevBuf tmp;
  NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)count, st));
  NFM_TRY(tmp.alloc(bytes));
  NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, (int)count, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // tmp goes back to the block cache on return
  return NFM_OK;
}

// a copy kernel in the widest words both pointers allow (every array here is made of 4- or 8-byte elements)
int dsop_copy(nfm_ctx* ctx, void* dst, const void* src, size_t bytes) {
  hipStream_t st = ctx->stream;
  const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
  size_t done = 0;
  if (both % 16 == 0 && bytes >= 16) {
    const int64_t n = (int64_t)(bytes / 16);
    DS_LAUNCH(k_copy<uint4>, dsop_grid(ctx, n), n, (const uint4*)src, (uint4*)dst);
    done = (size_t)n * 16;
  } else if (both % 8 == 0 && bytes >= 8) {
    const int64_t n = (int64_t)(bytes / 8);
    DS_LAUNCH(k_copy<uint64_t>, dsop_grid(ctx, n), n, (const uint64_t*)src, (uint64_t*)dst);
    done = (size_t)n * 8;
  }
  if (done < bytes) {
    const int64_t n = (int64_t)((bytes - done) / 4);
    DS_LAUNCH(k_copy<uint32_t>, dsop_grid(ctx, n), n, (const uint32_t*)((const char*)src + done), (uint32_t*)((char*)dst + done));
  }
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// room for the entry arrays (at least one element each, as the loaders allocate them)
int dsop_alloc_entries(DsParts* out, int64_t nnz, bool with_fields) {
  const size_t e = (size_t)std::max<int64_t>(nnz, 1);
  NFM_TRY(out->indices.alloc(sizeof(int32_t) * e));
  NFM_TRY(out->data.alloc(sizeof(double) * e));
  if (with_fields) NFM_TRY(out->fields.alloc(sizeof(int32_t) * e));
  out->has_fields = with_fields;
  out->nnz = nnz;
  return NFM_OK;
}

int dsop_select_rows(nfm_ctx* ctx, const CsrView& X, const int64_t* rows_host, int64_t begin, int64_t m, DsParts* out) {
  hipStream_t st = ctx->stream;
  DevBuf rows, len, mx;
  NFM_TRY(len.alloc(sizeof(int64_t) * (m + 1)));
  NFM_TRY(mx.alloc(sizeof(int)));
  NFM_HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(int), st));
  if (rows_host) {
    NFM_TRY(rows.alloc(sizeof(int64_t) * m));
    NFM_HIP_CHECK(hipMemcpyAsync(rows.p, rows_host, sizeof(int64_t) * m, hipMemcpyHostToDevice, st));
  }
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (m + 1)));
  out->has_y = X.y != nullptr;
  if (out->has_y) NFM_TRY(out->y.alloc(sizeof(double) * m));
  DS_LAUNCH(k_sel_len, dsop_grid(ctx, m + 1), m, rows.as<int64_t>(), begin, X.indptr, X.y, len.as<int64_t>(), out->y.as<double>(),
            mx.as<int>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(dsop_exclusive_scan(st, len.as<int64_t>(), out->indptr.as<int64_t>(), m + 1));
  int64_t nnz = 0, base = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&nnz, out->indptr.as<int64_t>() + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipMemcpyAsync(&out->max_row, mx.p, sizeof(int), hipMemcpyDeviceToHost, st));
  if (!rows_host) NFM_HIP_CHECK(hipMemcpyAsync(&base, X.indptr + begin, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  NFM_TRY(dsop_alloc_entries(out, nnz, X.fields != nullptr));
  if (!rows_host) {  // a slice is one contiguous piece of every array
    NFM_TRY(dsop_copy(ctx, out->indices.p, X.indices + base, sizeof(int32_t) * nnz));
    NFM_TRY(dsop_copy(ctx, out->data.p, X.data + base, sizeof(double) * nnz));
    if (X.fields) NFM_TRY(dsop_copy(ctx, out->fields.p, X.fields + base, sizeof(int32_t) * nnz));
  } else if (nnz) {
    auto launch = [&](auto G) {
      DS_LAUNCH(k_sel_rows<G()>, dsop_grid(ctx, m, kBlock / G()), m, out->indptr.as<int64_t>(), rows.as<int64_t>(), X.indptr, X.indices, X.data,
                X.fields, out->indices.as<int32_t>(), out->data.as<double>(), out->fields.as<int32_t>());
    };
    if (nnz / m >= kWave) launch(std::integral_constant<int, kWave>{}); else launch(std::integral_constant<int, kG>{});
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // rows and len go back to the block cache on return
  out->n = m;
  out->d = X.d;
  out->n_fields = X.n_fields;
  return NFM_OK;
}

int dsop_vstack(nfm_ctx* ctx, const CsrView* parts, int n_parts, DsParts* out) {
  hipStream_t st = ctx->stream;
  int64_t n = 0, nnz = 0, n_fields = 0;
  int max_row = 0;
  bool has_y = true;
  for (int p = 0; p < n_parts; ++p) {
    n += parts[p].n;
    nnz += parts[p].nnz;
    n_fields = std::max<int64_t>(n_fields, parts[p].n_fields);
    max_row = std::max<int>(max_row, parts[p].max_row);
    has_y = has_y && parts[p].y != nullptr;
  }
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (n + 1)));
  NFM_TRY(dsop_alloc_entries(out, nnz, parts[0].fields != nullptr));
  out->has_y = has_y;
  if (has_y) NFM_TRY(out->y.alloc(sizeof(double) * std::max<int64_t>(n, 1)));
  int64_t r0 = 0, q0 = 0;
  for (int p = 0; p < n_parts; ++p) {
    const CsrView& X = parts[p];
    // rows r0 .. r0 + X.n and the closing element; the next part rewrites that element with the same value
    DS_LAUNCH(k_shift_ptr, dsop_grid(ctx, X.n + 1), X.n, X.indptr, q0, out->indptr.as<int64_t>() + r0);
    NFM_HIP_CHECK(hipGetLastError());
    NFM_TRY(dsop_copy(ctx, out->indices.as<int32_t>() + q0, X.indices, sizeof(int32_t) * X.nnz));
    NFM_TRY(dsop_copy(ctx, out->data.as<double>() + q0, X.data, sizeof(double) * X.nnz));
    if (out->has_fields) NFM_TRY(dsop_copy(ctx, out->fields.as<int32_t>() + q0, X.fields, sizeof(int32_t) * X.nnz));
    if (has_y) NFM_TRY(dsop_copy(ctx, out->y.as<double>() + r0, X.y, sizeof(double) * X.n));
    r0 += X.n;
    q0 += X.nnz;
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  out->n = n;
  out->d = parts[0].d;
  out->n_fields = out->has_fields ? n_fields : 0;
  out->max_row = max_row;
  return NFM_OK;
}

int dsop_hstack(nfm_ctx* ctx, const CsrView* parts, int n_parts, DsParts* out) {
  hipStream_t st = ctx->stream;
  const int64_t n = parts[0].n;
  DevBuf len, cur, mx;
  NFM_TRY(len.alloc(sizeof(int64_t) * (n + 1)));
  NFM_TRY(cur.alloc(sizeof(int64_t) * std::max<int64_t>(n, 1)));
  NFM_TRY(mx.alloc(sizeof(int)));
  NFM_HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(int), st));
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (n + 1)));
  int64_t nnz = 0, d = 0, n_fields = 0;
  for (int p = 0; p < n_parts; ++p) {
    DS_LAUNCH(k_hs_len, dsop_grid(ctx, n + 1), n, parts[p].indptr, len.as<int64_t>(), p == 0, p == n_parts - 1, mx.as<int>());
    NFM_HIP_CHECK(hipGetLastError());
    nnz += parts[p].nnz;
  }
  NFM_TRY(dsop_exclusive_scan(st, len.as<int64_t>(), out->indptr.as<int64_t>(), n + 1));
  NFM_HIP_CHECK(hipMemcpyAsync(&out->max_row, mx.p, sizeof(int), hipMemcpyDeviceToHost, st));
  NFM_TRY(dsop_copy(ctx, cur.p, out->indptr.p, sizeof(int64_t) * n));
  NFM_TRY(dsop_alloc_entries(out, nnz, parts[0].fields != nullptr));
  for (int p = 0; p < n_parts; ++p) {
    const CsrView& X = parts[p];
    if (X.nnz) {
      auto launch = [&](auto G) {
        DS_LAUNCH(k_hs_rows<G()>, dsop_grid(ctx, n, kBlock / G()), n, X.indptr, X.indices, X.data, X.fields, cur.as<int64_t>(), (int32_t)d,
                  (int32_t)n_fields, out->indices.as<int32_t>(), out->data.as<double>(), out->fields.as<int32_t>());
      };
      if (X.nnz / n >= kWave) launch(std::integral_constant<int, kWave>{}); else launch(std::integral_constant<int, kG>{});
      if (p + 1 < n_parts) DS_LAUNCH(k_hs_advance, dsop_grid(ctx, n), n, X.indptr, cur.as<int64_t>());
      NFM_HIP_CHECK(hipGetLastError());
    }
    d += X.d;
    n_fields += X.n_fields;
  }
  out->has_y = parts[0].y != nullptr;
  if (out->has_y) {
    NFM_TRY(out->y.alloc(sizeof(double) * std::max<int64_t>(n, 1)));
    NFM_TRY(dsop_copy(ctx, out->y.p, parts[0].y, sizeof(double) * n));
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  out->n = n;
  out->d = d;
  out->n_fields = out->has_fields ? n_fields : 0;
  return NFM_OK;
}

template <int NORM>
static int normalize_into(nfm_ctx* ctx, const CsrView& X, int axis, double* dst) {
  hipStream_t st = ctx->stream;
  if (axis == 1) {
    DS_LAUNCH(k_norm_rows<NORM>, dsop_grid(ctx, X.n, kGroups), X.n, X.indptr, X.data, dst);
    NFM_HIP_CHECK(hipGetLastError());
    return NFM_OK;
  }
  // axis 0: the reference adds a column's entries as it meets them walking the arrays front to back (tensor/sparse.nim:
  // 388-389).  A STABLE sort of the storage positions by column id lists every column's entries in that order, also when a
  // row repeats an id.
  NFM_CHECK(X.nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "normalize(axis=0) with more than 2^31-2 entries");
  DevBuf pos, spos, skey, cptr, norms, tmp;
  NFM_TRY(pos.alloc(sizeof(int32_t) * X.nnz));
  NFM_TRY(spos.alloc(sizeof(int32_t) * X.nnz));
  NFM_TRY(skey.alloc(sizeof(int32_t) * X.nnz));
  NFM_TRY(cptr.alloc(sizeof(int64_t) * (X.d + 1)));
  NFM_TRY(norms.alloc(sizeof(double) * std::max<int64_t>(X.d, 1)));
  DS_LAUNCH(k_iota32, dsop_grid(ctx, X.nnz), X.nnz, pos.as<int32_t>());
  int end_bit = 1;
  while (end_bit < 31 && ((int64_t)1 << end_bit) < X.d) ++end_bit;
  size_t bytes = 0;
  NFM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, X.indices, skey.as<int32_t>(), pos.as<int32_t>(), spos.as<int32_t>(),
                                                   (int)X.nnz, 0, end_bit, st));
  NFM_TRY(tmp.alloc(bytes));
  NFM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, X.indices, skey.as<int32_t>(), pos.as<int32_t>(), spos.as<int32_t>(),
                                                   (int)X.nnz, 0, end_bit, st));
  DS_LAUNCH(k_col_ptr, dsop_grid(ctx, X.d + 1), X.d, skey.as<int32_t>(), X.nnz, cptr.as<int64_t>());
  DS_LAUNCH(k_norm_cols<NORM>, dsop_grid(ctx, X.d, kGroups), X.d, cptr.as<int64_t>(), spos.as<int32_t>(), X.data, norms.as<double>());
  DS_LAUNCH(k_div_cols, dsop_grid(ctx, X.nnz), X.nnz, X.indices, X.data, norms.as<double>(), dst);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_HIP_CHECK(hipStreamSynchronize(st));  // the scratch goes back to the block cache on return
  return NFM_OK;
}

int dsop_normalize(nfm_ctx* ctx, const CsrView& X, int axis, int norm, DsParts* out) {
  hipStream_t st = ctx->stream;
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (X.n + 1)));
  NFM_TRY(dsop_alloc_entries(out, X.nnz, X.fields != nullptr));
  NFM_TRY(dsop_copy(ctx, out->indptr.p, X.indptr, sizeof(int64_t) * (X.n + 1)));
  NFM_TRY(dsop_copy(ctx, out->indices.p, X.indices, sizeof(int32_t) * X.nnz));
  if (X.fields) NFM_TRY(dsop_copy(ctx, out->fields.p, X.fields, sizeof(int32_t) * X.nnz));
  out->has_y = X.y != nullptr;
  if (out->has_y) {
    NFM_TRY(out->y.alloc(sizeof(double) * std::max<int64_t>(X.n, 1)));
    NFM_TRY(dsop_copy(ctx, out->y.p, X.y, sizeof(double) * X.n));
  }
  if (X.nnz) {
    double* dst = out->data.as<double>();
    NFM_TRY(norm == NORM_L1   ? normalize_into<NORM_L1>(ctx, X, axis, dst)
            : norm == NORM_L2 ? normalize_into<NORM_L2>(ctx, X, axis, dst)
                              : normalize_into<NORM_LINFTY>(ctx, X, axis, dst));
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  out->n = X.n;
  out->d = X.d;
  out->n_fields = X.n_fields;
  out->max_row = X.max_row;
  return NFM_OK;
}

int dsop_user_item(nfm_ctx* ctx, const char* path, const char* mem, int64_t mem_len, DsParts* out, bool short_lines) {
  hipStream_t st = ctx->stream;
  hipEvent_t e0, e1, e2;
  NFM_HIP_CHECK(hipEventCreate(&e0));
  NFM_HIP_CHECK(hipEventCreate(&e1));
  NFM_HIP_CHECK(hipEventCreate(&e2));
  struct EvGuard {
    hipEvent_t a, b, c;
    ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); (void)hipEventDestroy(c); }
  } guard{e0, e1, e2};
  NFM_HIP_CHECK(hipEventRecord(e0, st));
  DevBuf text;
  int64_t len = 0;
  if (path) {
    NFM_TRY(upload_file(ctx, path, &text, &len));
  } else {
    NFM_CHECK(mem || mem_len == 0, NFM_ERR_INVALID, "null text");
    len = mem_len;
    NFM_TRY(text.alloc((size_t)len + 64));
    if (len) NFM_HIP_CHECK(hipMemcpyAsync(text.p, mem, (size_t)len, hipMemcpyHostToDevice, st));
  }
  NFM_HIP_CHECK(hipEventRecord(e1, st));
  DevBuf nl, co, table, status, keep, rowof, user, item, rating;
  int64_t n_nl = 0, n_co = 0, n_lines = 0;
  NFM_TRY(text_line_index(ctx, text.as<char>(), len, &nl, &co, &n_nl, &n_co, &n_lines));
  NFM_TRY(upload_pow5_table(ctx, &table));
  long long h_st[UI_COUNT] = {0, INT64_MAX, INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN, 0, 0};
  NFM_TRY(status.alloc(sizeof(h_st)));
  NFM_HIP_CHECK(hipMemcpyAsync(status.p, h_st, sizeof(h_st), hipMemcpyHostToDevice, st));
  const size_t nl1 = (size_t)n_lines + 1;
  NFM_TRY(keep.alloc(sizeof(int64_t) * nl1));
  NFM_TRY(rowof.alloc(sizeof(int64_t) * nl1));
  NFM_TRY(user.alloc(sizeof(int64_t) * nl1));
  NFM_TRY(item.alloc(sizeof(int64_t) * nl1));
  NFM_TRY(rating.alloc(sizeof(double) * nl1));
  DS_LAUNCH(k_ui_lines, dsop_grid(ctx, n_lines + 1), text.as<char>(), len, nl.as<int64_t>(), n_nl, n_lines, table.as<num::Pow5>(),
            keep.as<int64_t>(), user.as<int64_t>(), item.as<int64_t>(), rating.as<double>(), status.as<long long>(), short_lines ? 5 : 4);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(dsop_exclusive_scan(st, keep.as<int64_t>(), rowof.as<int64_t>(), n_lines + 1));
  int64_t n_rows = 0;
  NFM_HIP_CHECK(hipMemcpyAsync(&n_rows, rowof.as<int64_t>() + n_lines, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipMemcpyAsync(h_st, status.p, sizeof(h_st), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  NFM_CHECK(h_st[UI_BAD] == 0, NFM_ERR_INVALID,
            "malformed user-item-rating text: %lld lines without `user item rating`, first at line %lld", h_st[UI_BAD], h_st[UI_FIRST_BAD] + 1);
  NFM_CHECK(h_st[UI_LONG] == 0, NFM_ERR_UNSUPPORTED, "%lld ratings with more than 19 significant digits", h_st[UI_LONG]);
  NFM_CHECK(n_rows >= 1, NFM_ERR_INVALID, "no `user item rating` line in the text");
  // dataset.nim:863-867: the minima start at 1 and the maxima at 0
  const int64_t min_user = std::min<int64_t>(1, h_st[UI_MIN_USER]), max_user = std::max<int64_t>(0, h_st[UI_MAX_USER]);
  const int64_t min_item = std::min<int64_t>(1, h_st[UI_MIN_ITEM]), max_item = std::max<int64_t>(0, h_st[UI_MAX_ITEM]);
  const int64_t n_users = max_user - min_user + 1, n_items = max_item - min_item + 1;
  NFM_CHECK(n_users + n_items < (int64_t)2147483647 - 64, NFM_ERR_INVALID, "user and item ids up to %lld and %lld do not fit int32",
            (long long)max_user, (long long)max_item);
  NFM_TRY(out->indptr.alloc(sizeof(int64_t) * (n_rows + 1)));
  NFM_TRY(dsop_alloc_entries(out, 2 * n_rows, false));
  NFM_TRY(out->y.alloc(sizeof(double) * n_rows));
  out->has_y = true;
  DS_LAUNCH(k_ui_fill, dsop_grid(ctx, n_lines + 1), n_lines, n_rows, keep.as<int64_t>(), rowof.as<int64_t>(), user.as<int64_t>(),
            item.as<int64_t>(), rating.as<double>(), min_user, n_users - min_item, out->indptr.as<int64_t>(), out->indices.as<int32_t>(),
            out->data.as<double>(), out->y.as<double>());
  NFM_HIP_CHECK(hipGetLastError());
  NFM_HIP_CHECK(hipEventRecord(e2, st));
  NFM_HIP_CHECK(hipEventSynchronize(e2));
  float ms_up = 0, ms_parse = 0;
  NFM_HIP_CHECK(hipEventElapsedTime(&ms_up, e0, e1));
  NFM_HIP_CHECK(hipEventElapsedTime(&ms_parse, e1, e2));
  out->n = n_rows;
  out->d = n_users + n_items;
  out->n_fields = 0;
  out->max_row = 2;
  out->bytes = len;
  out->upload_ms = ms_up;
  out->parse_ms = ms_parse;
  return NFM_OK;
}

}  // namespace nfm
