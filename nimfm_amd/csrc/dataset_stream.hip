// nimfm_amd/csrc/dataset_stream.hip -- a compressed matrix in HBM -> the bytes of its binary stream file (DESIGN.md
// section 30): the inverse of ingest.hip's k_stream_split.
//
// The format (tensor/sparse_stream.nim:3-33):
//   magic "STREAMCSR" / "STREAMCSC" (9 bytes) | {nRows, nCols, nnz: int64; max, min: float64} |
//   per record: count: int64, then count x {val: float64, id: int64}
//   magic "STREAMCSRFIELD" (14 bytes) | {nRows, nCols, nnz, nFields: int64; max, min} |
//   per record: count: int64, then count x {field: int64, val: float64, id: int64}
// The magic and the header (49 / 62 bytes) are written by the host.  Everything after them is a sequence of 8-byte WORDS:
// with E = 2 (3 with fields) words per element, record r begins at word pos(r) = r + E * indptr[r] of the body -- strictly
// increasing in r -- and its element e at word pos(r) + 1 + E * e.
//
// The body is cut at record boundaries into pieces of at most chunk_bytes (stream_pieces.h) and every piece is packed into a
// 16-byte aligned staging buffer from its word 0 on, so the 16-byte vector v of a piece holds its words 2v and 2v + 1 and no
// store is unaligned.  k_pack_stream is output-centric: a workgroup owns an aligned tile of kTileWords words.  It finds the
// record of the tile's first word by one binary search over pos(r), puts the starts of the records that begin inside the tile
// into LDS (relative to the tile, 4 bytes each), and every lane resolves its two words -- count, val, id or field -- by a
// search of that list, widens the int32 ids / fields to int64 in registers and issues one 16-byte store.  Consecutive lanes
// store consecutive vectors.  The pieces leave through dataset_text.hip's pipeline (dump_pipe.h): the copy to the host and
// the write() of piece p run beside the packing of piece p + 1.
#include <math.h>
#include <string.h>

#include <vector>

#include "dataset_stream.h"
#include "dump_pipe.h"
#include "stream_pieces.h"

namespace nfm {
namespace {

constexpr int kTileWords = 2048;                       // 16 KiB of output per workgroup and pass
constexpr int kVecPerLane = kTileWords / 2 / kBlock;   // 4 stores of 16 bytes per lane

inline unsigned grid_for(const nfm_ctx* ctx, int64_t n, int per) {
  int64_t b = (n + per - 1) / per;
  const int64_t cap = (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

// ptr: the piece's slice of indptr (n_r + 1 values); idx, fld, val: its entries (n_e of them); out: n_vec vectors of two words.
// n_words = n_r + E * n_e; when that is odd the last vector's second word is written as 0 (it is not part of the piece).
template <int E>
__global__ __launch_bounds__(kBlock) void k_pack_stream(int64_t n_r, int64_t n_e, const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ fld,
                                                        const double* __restrict__ val, int64_t id_add, int64_t field_add,
                                                        ulonglong2* __restrict__ out, int64_t n_vec) {
  __shared__ int32_t rel[kTileWords + 1];  // rel[i]: where record r_s + i begins, relative to the tile; kTileWords: not inside
  const int tid = threadIdx.x;
  const int64_t e0 = ptr[0], n_words = n_r + (int64_t)E * n_e, n_tiles = (n_words + kTileWords - 1) / kTileWords;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t s = tile * kTileWords;
    // the record of the tile's first word: the last r with pos(r) = r + E * (ptr[r] - e0) <= s (pos(0) = 0)
    int64_t lo = 0, hi = n_r - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (mid + (int64_t)E * (ptr[mid] - e0) <= s) lo = mid; else hi = mid - 1;
    }
    const int64_t r_s = lo, pos_s = r_s + (int64_t)E * (ptr[r_s] - e0);
    for (int i = tid; i <= kTileWords; i += kBlock) {  // at most kTileWords more records begin inside the tile
      const int64_t r = r_s + i;
      int32_t v = kTileWords;
      if (i == 0) {
        v = 0;  // begins at or before the tile: pos_s
      } else if (r < n_r) {
        const int64_t p = r + (int64_t)E * (ptr[r] - e0) - s;
        if (p < kTileWords) v = (int32_t)p;
      }
      rel[i] = v;
    }
    __syncthreads();
    // word lw of the tile, which lies in record r_s + i
    auto word = [&](int i, int lw) -> unsigned long long {
      const int64_t r = r_s + i, p = i == 0 ? pos_s : s + rel[i], off = s + lw - p;
      if (off == 0) return (unsigned long long)(ptr[r + 1] - ptr[r]);
      const int64_t k = off - 1, e = k / E, el = (p - r) / E + e;
      const int m = (int)(k - e * E);
      if (el < 0 || el >= n_e) return 0ull;  // (an indptr that does not describe the piece)
      if (m == E - 1) return (unsigned long long)((int64_t)idx[el] + id_add);
      if (m == E - 2) return (unsigned long long)__double_as_longlong(val[el]);
      return (unsigned long long)((int64_t)fld[el] + field_add);
    };
#pragma unroll
    for (int q = 0; q < kVecPerLane; ++q) {
      const int lv = q * kBlock + tid, lw = 2 * lv;
      const int64_t w = s + lw, v = (s >> 1) + lv;
      if (w < n_words && v < n_vec) {
        int a = 0, b = kTileWords;  // the last i with rel[i] <= lw
        while (a < b) {
          const int mid = (a + b + 1) >> 1;
          if (rel[mid] <= lw) a = mid; else b = mid - 1;
        }
        ulonglong2 o;
        o.x = word(a, lw);
        o.y = 0ull;
        if (w + 1 < n_words) o.y = word(rel[a + 1] == lw + 1 ? a + 1 : a, lw + 1);  // (a < kTileWords: pos(r_s + i) >= s + i)
        out[v] = o;
      }
    }
    __syncthreads();  // rel is rewritten by the next pass
  }
}

// ---- the header's max / min ------------------------------------------------------------------------------------------------
// The fold v < vmin ? v : vmin from +Inf keeps the FIRST of the values that compare equal to the minimum and never a NaN.  In
// any order that is: of two candidates the smaller wins, and of two that compare equal the one earlier in storage.
struct MinMax {
  double mn, mx;
  int64_t imn, imx;  // -1: the seed, before every value
};
__host__ __device__ inline void mm_merge(MinMax& a, const MinMax& b) {
  if (b.mn < a.mn || (b.mn == a.mn && b.imn < a.imn)) { a.mn = b.mn; a.imn = b.imn; }
  if (b.mx > a.mx || (b.mx == a.mx && b.imx < a.imx)) { a.mx = b.mx; a.imx = b.imx; }
}

__global__ __launch_bounds__(kBlock) void k_minmax(int64_t n, const double* __restrict__ val, MinMax* __restrict__ part) {
  __shared__ MinMax sh[kBlock];
  MinMax m{HUGE_VAL, -HUGE_VAL, -1, -1};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = val[i];
    if (v < m.mn) { m.mn = v; m.imn = i; }  // i ascends: an equal value later in storage never replaces
    if (v > m.mx) { m.mx = v; m.imx = i; }
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) mm_merge(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

}  // namespace

int stream_minmax(nfm_ctx* ctx, const double* data, int64_t nnz, double* vmax, double* vmin) {
  MinMax m{HUGE_VAL, -HUGE_VAL, -1, -1};  // Nim's high(float64) / low(float64) are +-Inf
  if (nnz > 0) {
    hipStream_t st = ctx->stream;
    const unsigned grid = grid_for(ctx, nnz, kBlock * 8);
    DevBuf part;
    NFM_TRY(part.alloc(sizeof(MinMax) * grid));
    {
      TimedLaunch tl(ctx, "stream_minmax");
      hipLaunchKernelGGL(k_minmax, dim3(grid), dim3(kBlock), 0, st, nnz, data, part.as<MinMax>());
    }
    NFM_HIP_CHECK(hipGetLastError());
    std::vector<MinMax> h(grid);
    NFM_HIP_CHECK(hipMemcpyAsync(h.data(), part.p, sizeof(MinMax) * grid, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    for (const MinMax& p : h) mm_merge(m, p);
  }
  *vmax = m.mx;
  *vmin = m.mn;
  return NFM_OK;
}

int stream_head(int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_fields, double vmax, double vmin, char* head) {
  const char* magic = kind == STREAM_CSRFIELD ? "STREAMCSRFIELD" : kind == STREAM_CSC ? "STREAMCSC" : "STREAMCSR";
  int at = (int)strlen(magic);
  memcpy(head, magic, (size_t)at);
  auto put = [&](const void* p) {
    memcpy(head + at, p, 8);
    at += 8;
  };
  put(&n_rows);
  put(&n_cols);
  put(&nnz);
  if (kind == STREAM_CSRFIELD) put(&n_fields);
  put(&vmax);
  put(&vmin);
  return at;
}

int pack_stream(nfm_ctx* ctx, const CsrView& X, int64_t id_add, int64_t field_add, const char* head, int head_len, int64_t chunk_bytes,
                const TextSink& sink, int64_t* len_out, TextStats* stats) {
  hipStream_t st = ctx->stream;
  const double t_begin = dump_now_ms();
  const int64_t n = X.n;
  const int E = X.fields ? 3 : 2, esize = 8 * E;
  const bool length_only = sink.fd < 0 && !sink.buf;
  *len_out = 0;
  if (stats) *stats = TextStats();
  std::vector<int64_t> ip((size_t)n + 1, 0);
  if (n > 0) {
    NFM_HIP_CHECK(hipMemcpyAsync(ip.data(), X.indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  const StreamPieces pieces = stream_pieces(ip.data(), n, esize, chunk_bytes);
  const int64_t total = head_len + pieces.total_bytes, n_pieces = pieces.n_pieces();
  *len_out = total;
  if (stats) {
    stats->pieces = n_pieces;
    stats->bytes = total;
  }
  if (length_only) {
    if (stats) stats->total_ms = dump_now_ms() - t_begin;
    return NFM_OK;
  }
  NFM_CHECK(!sink.buf || total <= sink.cap, NFM_ERR_INVALID, "the buffer holds %lld bytes, the file is longer", (long long)sink.cap);
  DumpPipe P;
  P.ctx = ctx;
  const int64_t out_cap = (pieces.max_bytes + 15) / 16 * 16 + 16;
  NFM_TRY(P.open(ctx, sink, out_cap, false));
  NFM_TRY(P.put(head, head_len));
  for (int64_t p = 0; p < n_pieces; ++p) {
    DumpPipe::Slot& S = P.slot[p & 1];
    const int64_t r0 = pieces.cut[p], r1 = pieces.cut[p + 1], n_r = r1 - r0, e0 = ip[r0], n_e = ip[r1] - e0;
    const int64_t n_words = n_r + (int64_t)E * n_e, n_vec = (n_words + 1) / 2;
    NFM_CHECK(n_vec * 16 <= out_cap, NFM_ERR_HIP, "a piece of %lld bytes where at most %lld fit", (long long)(n_words * 8), (long long)out_cap);
    {
      TimedLaunch tl(ctx, "stream_pack");
      const unsigned grid = grid_for(ctx, n_words, kTileWords);
      if (E == 3)
        hipLaunchKernelGGL(k_pack_stream<3>, dim3(grid), dim3(kBlock), 0, st, n_r, n_e, X.indptr + r0, X.indices + e0, X.fields + e0,
                           X.data + e0, id_add, field_add, S.out.as<ulonglong2>(), n_vec);
      else
        hipLaunchKernelGGL(k_pack_stream<2>, dim3(grid), dim3(kBlock), 0, st, n_r, n_e, X.indptr + r0, X.indices + e0,
                           (const int32_t*)nullptr, X.data + e0, id_add, field_add, S.out.as<ulonglong2>(), n_vec);
    }
    NFM_HIP_CHECK(hipGetLastError());
    NFM_HIP_CHECK(hipEventRecord(S.fmt, st));
    NFM_TRY(P.consume(P.slot[(p & 1) ^ 1]));  // piece p - 1 leaves while piece p is packed
    NFM_HIP_CHECK(hipEventSynchronize(S.fmt));
    S.len = n_words * 8;
    NFM_TRY(P.send(S));
  }
  if (n_pieces > 0) NFM_TRY(P.consume(P.slot[(n_pieces - 1) & 1]));
  if (stats) {
    stats->copy_ms = P.copy_ms;
    stats->sink_ms = P.sink_ms;
    stats->total_ms = dump_now_ms() - t_begin;
  }
  return NFM_OK;
}

}  // namespace nfm
