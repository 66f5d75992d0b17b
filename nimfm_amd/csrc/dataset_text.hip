// nimfm_amd/csrc/dataset_text.hip -- a dataset in HBM -> the bytes of its text file: the inverse of
// ingest.hip.
//
// Replaces, for a dataset resident on the device, the reference's host-side writers
//   dumpSVMLightFile   dataset.nim:793-805     row i: y_i, then " (j+1):val" per entry
//   dumpFFMFile        dataset.nim:825-837     row i: y_i, then " (field+1):(j+1):val" per entry
// ("\n" between rows, none after the last; ids 1-based; numbers as format_num.h writes them), and the number blocks of the
// model dump (model/factorization_machine.nim:142-165).
//
// The rows are walked in pieces whose text is at most chunk_bytes (a piece is cut from indptr by the longest its rows can
// be -- 25 bytes of row header, 36 / 47 bytes per entry -- so no number is converted to find the cuts; a row longer than
// chunk_bytes is a piece by itself).  Per piece, on the context's stream:
//   1. length pass: every value -> its shortest decimal (format_num.h decompose), kept in ten bytes per number, and the
//      length of its token; per row the length of its header ("\n" except on the first row of the file, then y_i);
//   2. two int64 exclusive scans (hipcub): entry tokens, row headers.  The header of row r starts at hoff[r] + eoff[ptr[r]],
//      entry e of row r at hoff[r + 1] + eoff[e]: every byte has one writer, no atomics;
//   3. write pass: headers and entries in file order are one sequence of ITEMS (header of row r: item ptr[r] + r); a
//      workgroup takes 256 consecutive items, whose tokens are one contiguous span of the text (at most 256 x 47 bytes).
//      Its rows are found together, not per item: one search for the row of the span's first item, then the 256 lanes mark
//      where the following rows begin and a max-scan hands every item its row.  Every lane writes its token (from the kept
//      decimal: no 128-bit product a second time) into the span in LDS, placed at the span's own offset modulo 16, and the
//      workgroup stores the span to global memory in aligned 16-byte words (up to 15 single bytes at either end).
// Two device buffers, two pinned host buffers and a copy stream: the copy out and the write() of piece p run beside the
// formatting of piece p + 1.  Every kernel is a grid-stride loop over at most n_cu * 8 workgroups of 256.
#include <hipcub/hipcub.hpp>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include "dataset_text.h"
#include "dump_pipe.h"
#include "format_num.h"

namespace nfm {
namespace {

using num::Dec;
using num::Pow;

const Pow kFmtHost[] = NFM_FMT_POW5_TABLE_INIT;
constexpr int kFmtN = NFM_FMT_N_INV + NFM_FMT_N_POW;

constexpr int kHeaderMax = 1 + num::kFmtMaxFloat;                // "\n" y
constexpr int kEntryMax = 1 + 10 + 1 + num::kFmtMaxFloat;        // " " id ":" val
constexpr int kEntryMaxFfm = kEntryMax + 10 + 1;                 // " " field ":" id ":" val
constexpr int kTokMax = kEntryMaxFfm;                            // 47
constexpr int kSpanBytes = kBlock * 48;                          // the tokens of 256 items
constexpr int64_t kDefaultChunk = (int64_t)128 << 20;
constexpr int64_t kMaxChunk = (int64_t)1 << 30;                  // keeps a piece's counts far below hipcub's 2^31 - 2 items

inline unsigned grid_for(const nfm_ctx* ctx, int64_t n, int per = kBlock) {
  int64_t b = (n + per - 1) / per;
  const int64_t cap = (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

#define DT_LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__)

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

// ---- length pass -----------------------------------------------------------------------------------------------------
// the entries [0, n_e) of a piece (the pointers are the piece's): decimal of the value, length of the token; len[n_e] = 0
__global__ __launch_bounds__(kBlock) void k_len_entries(int64_t n_e, const int32_t* __restrict__ idx, const int32_t* __restrict__ fld,
                                                        const double* __restrict__ val, const Pow* __restrict__ table,
                                                        uint64_t* __restrict__ sig, int16_t* __restrict__ ex, int64_t* __restrict__ len) {
  for (int64_t i = gtid(); i <= n_e; i += gstride()) {
    if (i == n_e) {
      len[i] = 0;
      continue;
    }
    const Dec d = num::decompose(val[i], table);
    num::pack_dec(d, &sig[i], &ex[i]);
    int l = 2 + num::dec_digits((uint64_t)(uint32_t)(idx[i] + 1)) + num::dec_length(d);
    if (fld) l += 1 + num::dec_digits((uint64_t)(uint32_t)(fld[i] + 1));
    len[i] = l;
  }
}

// the rows [0, n_r) of a piece: decimal of the target, length of the header; first: the piece begins the file
__global__ __launch_bounds__(kBlock) void k_len_rows(int64_t n_r, const double* __restrict__ y, int y_int, int first,
                                                     const Pow* __restrict__ table, uint64_t* __restrict__ sig, int16_t* __restrict__ ex,
                                                     int64_t* __restrict__ len, int* __restrict__ bad) {
  for (int64_t i = gtid(); i <= n_r; i += gstride()) {
    if (i == n_r) {
      len[i] = 0;
      continue;
    }
    const double v = y[i];
    Dec d;
    if (y_int) {
      const bool ok = v > -9007199254740992.0 && v < 9007199254740992.0 && v == (double)(int64_t)v;
      if (!ok) *bad = 1;  // (every writer stores the same value)
      d = num::dec_from_int(ok ? (int64_t)v : 0);
    } else {
      d = num::decompose(v, table);
    }
    num::pack_dec(d, &sig[i], &ex[i]);
    len[i] = ((first && i == 0) ? 0 : 1) + num::dec_length(d);
  }
}

// ---- write pass ------------------------------------------------------------------------------------------------------
// the span [start, start + total) of the text, built in LDS at buf[a ...] with a = start % 16, to out: aligned 16-byte
// words, single bytes at the ends.  out is 16-byte aligned; the caller has checked start + total <= the room at out.
__device__ __forceinline__ void flush_span(const char* buf, int a, int64_t start, int total, char* __restrict__ out) {
  const int tid = threadIdx.x;
  int head = (16 - a) & 15;
  if (head > total) head = total;
  const int words = (total - head) / 16, tail = total - head - words * 16;
  if (tid < head) out[start + tid] = buf[a + tid];
  const uint4* src = reinterpret_cast<const uint4*>(buf + a + head);
  uint4* dst = reinterpret_cast<uint4*>(out + start + head);
  if (words > 0)
    for (int w = tid; w < words; w += kBlock) dst[w] = src[w];
  if (tid < tail) out[start + head + words * 16 + tid] = buf[a + head + words * 16 + tid];
}

// inclusive maximum over the workgroup's lanes in lane order (wmax: kWavesPerBlock ints of LDS)
__device__ __forceinline__ int block_max_scan(int v, int* wmax) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  for (int o = 1; o < kWave; o <<= 1) {
    const int u = __shfl_up(v, o, kWave);
    if (lane >= o) v = u > v ? u : v;
  }
  if (lane == kWave - 1) wmax[w] = v;
  __syncthreads();
  for (int k = 0; k < w; ++k) v = wmax[k] > v ? wmax[k] : v;
  return v;
}

// ptr: the piece's slice of indptr (n_r + 1 values), e0 = ptr[0]; idx, fld, esig, eex, eoff: the piece's entries; ysig, yex,
// hoff: its rows; first: the piece begins the file.  out: the piece's text, room for out_cap bytes.
__global__ __launch_bounds__(kBlock) void k_write_items(int64_t n_r, int64_t n_e, const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ fld,
                                                        const uint64_t* __restrict__ esig, const int16_t* __restrict__ eex,
                                                        const int64_t* __restrict__ eoff, const uint64_t* __restrict__ ysig,
                                                        const int16_t* __restrict__ yex, const int64_t* __restrict__ hoff, int first,
                                                        char* __restrict__ out, int64_t out_cap) {
  __shared__ __align__(16) char buf[kSpanBytes + 16];
  __shared__ int mark[kBlock];
  __shared__ int wmax[kWavesPerBlock];
  __shared__ int64_t span_lo, span_hi;
  const int tid = threadIdx.x;
  const int64_t e0 = ptr[0], n_items = n_e + n_r, n_spans = (n_items + kBlock - 1) / kBlock;
  for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
    const int64_t s = span * kBlock, t = s + tid;
    // the row of the span's first item: the last r with item(r) = ptr[r] - e0 + r <= s (item(0) = 0)
    int64_t lo = 0, hi = n_r - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (ptr[mid] - e0 + mid <= s) lo = mid; else hi = mid - 1;
    }
    const int64_t r_s = lo;
    mark[tid] = 0;
    __syncthreads();
    {  // the rows that begin inside the span are among the next 256
      const int64_t r = r_s + 1 + tid;
      if (r < n_r) {
        const int64_t g = ptr[r] - e0 + r;
        if (g < s + kBlock) mark[(int)(g - s)] = tid + 1;
      }
    }
    __syncthreads();
    const int64_t row = r_s + block_max_scan(mark[tid], wmax);
    int64_t pos = 0;
    int len = 0;
    bool header = false;
    int64_t el = 0;
    if (t < n_items) {
      const int64_t pr = ptr[row] - e0;
      header = pr + row == t;
      if (header) {
        pos = hoff[row] + eoff[pr];
        len = (int)(hoff[row + 1] - hoff[row]);
      } else {
        el = t - (row + 1);
        pos = hoff[row + 1] + eoff[el];
        len = (int)(eoff[el + 1] - eoff[el]);
      }
      if (tid == 0) span_lo = pos;
      if (tid == kBlock - 1 || t == n_items - 1) span_hi = pos + len;
    }
    __syncthreads();
    const int64_t start = span_lo;
    const int a = (int)(start & 15);
    const int64_t total = span_hi - start;
    const int64_t rel = pos - start;
    if (t < n_items && len > 0 && len <= kTokMax && rel >= 0 && rel + len <= kSpanBytes) {
      char* p = buf + a + rel;
      if (header) {
        if (!(first && row == 0)) *p++ = '\n';
        num::dec_write(num::unpack_dec(ysig[row], yex[row]), p);
      } else {
        *p++ = ' ';
        if (fld) {
          p += num::format_uint((uint64_t)(uint32_t)(fld[el] + 1), p);
          *p++ = ':';
        }
        p += num::format_uint((uint64_t)(uint32_t)(idx[el] + 1), p);
        *p++ = ':';
        num::dec_write(num::unpack_dec(esig[el], eex[el]), p);
      }
    }
    __syncthreads();
    if (total > 0 && total <= kSpanBytes && start >= 0 && start + total <= out_cap) flush_span(buf, a, start, (int)total, out);
    __syncthreads();  // the span in LDS is reused by the next pass
  }
}

// ---- a block of numbers (the model dump) -----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_len_f64(int64_t m, const double* __restrict__ val, const Pow* __restrict__ table,
                                                    uint64_t* __restrict__ sig, int16_t* __restrict__ ex, int64_t* __restrict__ len) {
  for (int64_t i = gtid(); i <= m; i += gstride()) {
    if (i == m) {
      len[i] = 0;
      continue;
    }
    const Dec d = num::decompose(val[i], table);
    num::pack_dec(d, &sig[i], &ex[i]);
    len[i] = num::dec_length(d) + 1;
  }
}

// value i of the piece is value g0 + i of the block: "\n" after the last of a row, " " after the others
__global__ __launch_bounds__(kBlock) void k_write_f64(int64_t m, int64_t g0, int64_t row_len, const uint64_t* __restrict__ sig,
                                                      const int16_t* __restrict__ ex, const int64_t* __restrict__ off,
                                                      char* __restrict__ out, int64_t out_cap) {
  __shared__ __align__(16) char buf[kSpanBytes + 16];
  const int tid = threadIdx.x;
  const int64_t n_spans = (m + kBlock - 1) / kBlock;
  for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
    const int64_t s = span * kBlock, t = s + tid;
    const int64_t last = (s + kBlock < m ? s + kBlock : m);
    const int64_t start = off[s], total = off[last] - start;
    const int a = (int)(start & 15);
    if (t < m) {
      const int64_t rel = off[t] - start;
      const int len = (int)(off[t + 1] - off[t]);
      if (len > 0 && len <= num::kFmtMaxFloat + 1 && rel >= 0 && rel + len <= kSpanBytes) {
        char* p = buf + a + rel;
        p += num::dec_write(num::unpack_dec(sig[t], ex[t]), p);
        *p = (g0 + t + 1) % row_len == 0 ? '\n' : ' ';
      }
    }
    __syncthreads();
    if (total > 0 && total <= kSpanBytes && start >= 0 && start + total <= out_cap) flush_span(buf, a, start, (int)total, out);
    __syncthreads();
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
double now_ms() { return dump_now_ms(); }

int upload_fmt_table(nfm_ctx* ctx, DevBuf* table) {
  NFM_TRY(table->alloc(sizeof(Pow) * kFmtN));
  NFM_HIP_CHECK(hipMemcpyAsync(table->p, kFmtHost, sizeof(Pow) * kFmtN, hipMemcpyHostToDevice, ctx->stream));
  return NFM_OK;
}

struct ScanTmp {
  DevBuf tmp;
  size_t bytes = 0;
  int prepare(hipStream_t st, int64_t max_count) {
    NFM_CHECK(max_count < (int64_t)2147483646, NFM_ERR_UNSUPPORTED, "a piece of more than 2^31-2 items");
    NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int)max_count, st));
    return tmp.alloc(bytes ? bytes : 1);
  }
  int run(hipStream_t st, const int64_t* in, int64_t* out, int64_t count) {
    size_t b = bytes;
    NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, b, in, out, (int)count, st));
    return NFM_OK;
  }
};

// The two pinned host buffers, made once per process and grown when a call needs more (ingest.hip's UploadSlots, mirrored):
// pinning 2 x 128 MiB costs more than formatting a million rows.  One call at a time uses them.
struct PinnedPair {
  char* pin[2] = {nullptr, nullptr};
  size_t cap = 0;
  int device = -1;
  std::mutex mu;
};
PinnedPair& pinned_pair() {
  static PinnedPair* P = new PinnedPair();  // lives until process exit
  return *P;
}
int pinned_reserve(PinnedPair& P, int device, size_t bytes) {
  if (P.device == device && P.cap >= bytes) return NFM_OK;
  for (char*& p : P.pin) {
    if (p) (void)hipHostFree(p);
    p = nullptr;
  }
  P.cap = 0;
  P.device = device;
  for (char*& p : P.pin) NFM_HIP_CHECK(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
  P.cap = bytes;
  return NFM_OK;
}

int sink_write(const TextSink& sink, int64_t at, const char* p, int64_t len) {
  if (sink.buf) {
    memcpy(sink.buf + at, p, (size_t)len);
    return NFM_OK;
  }
  int64_t done = 0;
  while (done < len) {
    const ssize_t k = write(sink.fd, p + done, (size_t)(len - done));
    NFM_CHECK(k > 0, NFM_ERR_INVALID, "the text could not be written (%lld of %lld bytes of a piece)", (long long)done, (long long)len);
    done += k;
  }
  return NFM_OK;
}

}  // namespace

// ---- the two halves of the pipeline and what they share (dump_pipe.h); everything but the pinned pair is given back when
// the call ends, however it ends
double dump_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int DumpPipe::open(nfm_ctx* ctx_, const TextSink& sink_, int64_t out_cap, bool length_only) {
  ctx = ctx_;
  sink = sink_;
  if (!length_only) {
    PinnedPair& pinned = pinned_pair();
    NFM_HIP_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    pinned_lock = std::unique_lock<std::mutex>(pinned.mu);
    NFM_TRY(pinned_reserve(pinned, ctx->device, (size_t)out_cap));
    slot[0].pin = pinned.pin[0];
    slot[1].pin = pinned.pin[1];
  }
  for (Slot& s : slot) {
    NFM_HIP_CHECK(hipHostMalloc((void**)&s.tot, sizeof(int64_t) * 4, hipHostMallocDefault));
    NFM_HIP_CHECK(hipEventCreateWithFlags(&s.fmt, hipEventDisableTiming));
    if (length_only) continue;
    NFM_TRY(s.out.alloc((size_t)out_cap));
    NFM_HIP_CHECK(hipEventCreate(&s.c0));
    NFM_HIP_CHECK(hipEventCreate(&s.c1));
  }
  return NFM_OK;
}

int DumpPipe::put(const char* p, int64_t len) {
  const double t0 = dump_now_ms();
  NFM_TRY(sink_write(sink, written, p, len));
  sink_ms += dump_now_ms() - t0;
  written += len;
  return NFM_OK;
}

int DumpPipe::send(Slot& S) {
  NFM_HIP_CHECK(hipEventRecord(S.c0, copy_stream));
  NFM_HIP_CHECK(hipMemcpyAsync(S.pin, S.out.p, (size_t)S.len, hipMemcpyDeviceToHost, copy_stream));
  NFM_HIP_CHECK(hipEventRecord(S.c1, copy_stream));
  S.busy = true;
  return NFM_OK;
}

int DumpPipe::consume(Slot& s) {
  if (!s.busy) return NFM_OK;
  s.busy = false;
  NFM_HIP_CHECK(hipEventSynchronize(s.c1));
  float ms = 0.0f;
  NFM_HIP_CHECK(hipEventElapsedTime(&ms, s.c0, s.c1));
  copy_ms += ms;
  return put(s.pin, s.len);
}

DumpPipe::~DumpPipe() {
  if (copy_stream) (void)hipStreamSynchronize(copy_stream);
  if (ctx) (void)hipStreamSynchronize(ctx->stream);  // the device blocks go back to the cache
  for (Slot& s : slot) {
    if (s.tot) (void)hipHostFree(s.tot);
    if (s.fmt) (void)hipEventDestroy(s.fmt);
    if (s.c0) (void)hipEventDestroy(s.c0);
    if (s.c1) (void)hipEventDestroy(s.c1);
  }
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
}

int format_dataset_text(nfm_ctx* ctx, const CsrView& X, const double* y_host, bool y_int, int64_t chunk_bytes, const TextSink& sink,
                        int64_t* len_out, TextStats* stats) {
  hipStream_t st = ctx->stream;
  const double t_begin = now_ms();
  const int64_t n = X.n;
  const bool length_only = sink.fd < 0 && !sink.buf;
  *len_out = 0;
  if (stats) *stats = TextStats();
  if (n == 0) return NFM_OK;
  std::vector<int64_t> ip((size_t)n + 1);
  NFM_HIP_CHECK(hipMemcpyAsync(ip.data(), X.indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  // the cuts: the most a piece's rows can take stays within chunk (one row at least)
  const int64_t chunk = chunk_bytes > 0 ? std::min(chunk_bytes, kMaxChunk) : kDefaultChunk;
  const int64_t per_entry = X.fields ? kEntryMaxFfm : kEntryMax;
  std::vector<int64_t> cut{0};
  int64_t max_bound = 0, max_e = 0, max_r = 0;
  for (int64_t r = 0; r < n;) {
    int64_t bound = 0, r1 = r;
    while (r1 < n) {
      const int64_t b = kHeaderMax + (ip[r1 + 1] - ip[r1]) * per_entry;
      if (r1 > r && bound + b > chunk) break;
      bound += b;
      ++r1;
    }
    max_bound = std::max(max_bound, bound);
    max_e = std::max(max_e, ip[r1] - ip[r]);
    max_r = std::max(max_r, r1 - r);
    cut.push_back(r1);
    r = r1;
  }
  NFM_CHECK(max_e + max_r + 2 < (int64_t)2147483646, NFM_ERR_UNSUPPORTED, "a row of more than 2^31-2 entries");

  DevBuf table, ydev, esig, eex, elen, eoff, ysig, yex, hlen, hoff, bad;
  ScanTmp scan;
  DumpPipe P;  // destroyed first: both streams are drained before the blocks above go back to the cache and the lock is released
  P.ctx = ctx;
  NFM_TRY(upload_fmt_table(ctx, &table));
  const double* y = X.y;
  if (y_host) {
    NFM_TRY(ydev.alloc(sizeof(double) * n));
    NFM_HIP_CHECK(hipMemcpyAsync(ydev.p, y_host, sizeof(double) * n, hipMemcpyHostToDevice, st));
    y = ydev.as<double>();
  }
  NFM_TRY(esig.alloc(sizeof(uint64_t) * (max_e + 1)));
  NFM_TRY(eex.alloc(sizeof(int16_t) * (max_e + 1)));
  NFM_TRY(elen.alloc(sizeof(int64_t) * (max_e + 1)));
  NFM_TRY(eoff.alloc(sizeof(int64_t) * (max_e + 1)));
  NFM_TRY(ysig.alloc(sizeof(uint64_t) * (max_r + 1)));
  NFM_TRY(yex.alloc(sizeof(int16_t) * (max_r + 1)));
  NFM_TRY(hlen.alloc(sizeof(int64_t) * (max_r + 1)));
  NFM_TRY(hoff.alloc(sizeof(int64_t) * (max_r + 1)));
  NFM_TRY(bad.alloc(sizeof(int)));
  NFM_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  NFM_TRY(scan.prepare(st, std::max(max_e, max_r) + 1));
  const int64_t out_cap = max_bound + 16;
  NFM_TRY(P.open(ctx, sink, out_cap, length_only));

  int64_t total = 0;
  const int64_t n_pieces = (int64_t)cut.size() - 1;
  for (int64_t p = 0; p < n_pieces; ++p) {
    DumpPipe::Slot& S = P.slot[p & 1];
    const int64_t r0 = cut[p], r1 = cut[p + 1], n_r = r1 - r0, e0 = ip[r0], n_e = ip[r1] - e0;
    const int first = r0 == 0 ? 1 : 0;
    const int32_t* idx = X.indices + e0;
    const int32_t* fld = X.fields ? X.fields + e0 : nullptr;
    {
      TimedLaunch tl(ctx, "dump_len");
      DT_LAUNCH(k_len_entries, grid_for(ctx, n_e + 1), n_e, idx, fld, X.data + e0, table.as<Pow>(), esig.as<uint64_t>(), eex.as<int16_t>(),
                elen.as<int64_t>());
      DT_LAUNCH(k_len_rows, grid_for(ctx, n_r + 1), n_r, y + r0, y_int ? 1 : 0, first, table.as<Pow>(), ysig.as<uint64_t>(),
                yex.as<int16_t>(), hlen.as<int64_t>(), bad.as<int>());
    }
    NFM_HIP_CHECK(hipGetLastError());
    {
      TimedLaunch tl(ctx, "dump_scan");
      NFM_TRY(scan.run(st, elen.as<int64_t>(), eoff.as<int64_t>(), n_e + 1));
      NFM_TRY(scan.run(st, hlen.as<int64_t>(), hoff.as<int64_t>(), n_r + 1));
    }
    NFM_HIP_CHECK(hipMemcpyAsync(&S.tot[0], eoff.as<int64_t>() + n_e, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipMemcpyAsync(&S.tot[1], hoff.as<int64_t>() + n_r, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipMemcpyAsync(&S.tot[2], bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    if (!length_only) {
      TimedLaunch tl(ctx, "dump_write");
      DT_LAUNCH(k_write_items, grid_for(ctx, n_e + n_r), n_r, n_e, X.indptr + r0, idx, fld, esig.as<uint64_t>(), eex.as<int16_t>(),
                eoff.as<int64_t>(), ysig.as<uint64_t>(), yex.as<int16_t>(), hoff.as<int64_t>(), first, S.out.as<char>(), out_cap);
    }
    NFM_HIP_CHECK(hipGetLastError());
    NFM_HIP_CHECK(hipEventRecord(S.fmt, st));
    NFM_TRY(P.consume(P.slot[(p & 1) ^ 1]));  // piece p - 1 leaves while piece p is formatted
    NFM_HIP_CHECK(hipEventSynchronize(S.fmt));
    NFM_CHECK((int)S.tot[2] == 0, NFM_ERR_INVALID, "y_int: a target is not an integer below 2^53 in magnitude");
    S.len = S.tot[0] + S.tot[1];
    NFM_CHECK(S.len <= max_bound, NFM_ERR_HIP, "a piece of %lld bytes where at most %lld fit", (long long)S.len, (long long)max_bound);
    total += S.len;
    if (length_only) continue;
    NFM_CHECK(!sink.buf || total <= sink.cap, NFM_ERR_INVALID, "the buffer holds %lld bytes, the text is longer", (long long)sink.cap);
    NFM_TRY(P.send(S));
  }
  NFM_TRY(P.consume(P.slot[(n_pieces - 1) & 1]));
  *len_out = total;
  if (stats) {
    stats->copy_ms = P.copy_ms;
    stats->sink_ms = P.sink_ms;
    stats->total_ms = now_ms() - t_begin;
    stats->pieces = n_pieces;
    stats->bytes = total;
  }
  return NFM_OK;
}

int format_f64_text(nfm_ctx* ctx, const double* values, int64_t n_rows, int64_t row_len, char* buf, int64_t cap, int64_t* len_out) {
  hipStream_t st = ctx->stream;
  const int64_t count = n_rows * row_len;
  *len_out = 0;
  if (count == 0) return NFM_OK;
  const int64_t per = num::kFmtMaxFloat + 1;
  const int64_t piece = std::min(count, kDefaultChunk / per);
  DevBuf table, val, sig, ex, len, off, out;
  ScanTmp scan;
  struct Sync {  // the device blocks go back to the cache
    hipStream_t st;
    ~Sync() { (void)hipStreamSynchronize(st); }
  } sync{st};
  NFM_TRY(upload_fmt_table(ctx, &table));
  NFM_TRY(val.alloc(sizeof(double) * piece));
  NFM_TRY(sig.alloc(sizeof(uint64_t) * piece));
  NFM_TRY(ex.alloc(sizeof(int16_t) * piece));
  NFM_TRY(len.alloc(sizeof(int64_t) * (piece + 1)));
  NFM_TRY(off.alloc(sizeof(int64_t) * (piece + 1)));
  const int64_t out_cap = piece * per + 16;
  if (buf) NFM_TRY(out.alloc((size_t)out_cap));
  NFM_TRY(scan.prepare(st, piece + 1));
  int64_t total = 0;
  for (int64_t g0 = 0; g0 < count; g0 += piece) {
    const int64_t m = std::min(piece, count - g0);
    NFM_HIP_CHECK(hipMemcpyAsync(val.p, values + g0, sizeof(double) * m, hipMemcpyHostToDevice, st));
    DT_LAUNCH(k_len_f64, grid_for(ctx, m + 1), m, val.as<double>(), table.as<Pow>(), sig.as<uint64_t>(), ex.as<int16_t>(), len.as<int64_t>());
    NFM_HIP_CHECK(hipGetLastError());
    NFM_TRY(scan.run(st, len.as<int64_t>(), off.as<int64_t>(), m + 1));
    int64_t bytes = 0;
    NFM_HIP_CHECK(hipMemcpyAsync(&bytes, off.as<int64_t>() + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    NFM_CHECK(bytes <= m * per, NFM_ERR_HIP, "a piece of %lld bytes where at most %lld fit", (long long)bytes, (long long)(m * per));
    if (buf) {
      NFM_CHECK(total + bytes <= cap, NFM_ERR_INVALID, "the buffer holds %lld bytes, the text is longer", (long long)cap);
      DT_LAUNCH(k_write_f64, grid_for(ctx, m), m, g0, row_len, sig.as<uint64_t>(), ex.as<int16_t>(), off.as<int64_t>(), out.as<char>(), out_cap);
      NFM_HIP_CHECK(hipGetLastError());
      NFM_HIP_CHECK(hipMemcpyAsync(buf + total, out.p, (size_t)bytes, hipMemcpyDeviceToHost, st));
      NFM_HIP_CHECK(hipStreamSynchronize(st));
    }
    total += bytes;
  }
  *len_out = total;
  return NFM_OK;
}

}  // namespace nfm
