// nimfm_amd/csrc/model_text.hip -- the number blocks of a model dump, text -> float64 ON the GPU: the
// inverse of dataset_text.hip's format_f64_text, for `load` (model/factorization_machine.nim:168-220,
// field_aware_factorization_machine.nim:119-158, convex_factorization_machine.nim:111-164).
//
// The text goes up in pieces (model_text_pieces.h: cut at a separator, the last one ends with the block's n_rows-th '\n').
// Per piece, on the context's stream, in ingest.hip's pattern (a workgroup per 16-KiB tile, 64 bytes per thread as four
// 16-byte loads, exact byte masks, bytes past the piece never match):
//   1. k_mt_counts      '\n' and token starts per tile (a token starts at a byte that is no separator and follows one)
//   2. two int64 exclusive scans of the tile counts (hipcub); their last words are the piece's totals and stay on the device
//   3. k_mt_positions   the ascending positions of both, int32 inside the piece
//   4. k_mt_lines       one thread per '\n': the tokens of the line it ends (a line of fewer than row_len raises the status
//                       word); one more thread takes the open line at the piece's end and writes the carry for the next piece
//      k_mt_parse       one thread per token: its row by a search in the '\n' positions (plus the host's count of earlier
//                       lines), its column from the rank of its line's first token (plus the carried column on the piece's
//                       first line), parse_float, the store into the block's values in HBM
// Every launch is a grid-stride loop over data that is complete before it starts; nothing waits on another workgroup.
// What the device does not decide it reports: ST_BAD counts junk tokens and short lines, ST_FIX the tokens parse_float
// flags kNeedsStrtod, which the host re-reads with strtod from its own copy of the text.
//
// The way in is dump_pipe.h's DumpPipe run backwards: the pinned pair stages the text, the copy stream uploads piece p + 1
// and copies the values of piece p - 1 back while the context's stream parses piece p.  The column carry and the index of
// the next value live in device memory; the host learns the latter one piece late, from the pinned totals of the slot.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dump_pipe.h"
#include "ingest.h"  // upload_pow5_table
#include "model_text.h"
#include "model_text_pieces.h"

namespace nfm {
namespace {

using num::Pow5;

constexpr int kMtChunk = 64;               // bytes per thread
constexpr int kMtTile = kBlock * kMtChunk;  // bytes per workgroup (16 KiB)
constexpr int kMtGridCap = 1024;           // workgroups per launch
constexpr int kMtMaxFix = 1 << 20;         // tokens of one call the host may have to re-read

enum { ST_BAD = 0, ST_FIX = 1, ST_COUNT = 2 };

struct MtFix {
  int64_t pos;   // byte offset of the token in the call's text
  int64_t slot;  // index into values
};

// 0x80 in every byte of w that equals c (exact per byte; ingest.hip's)
__device__ __forceinline__ uint64_t eq_bytes(uint64_t w, uint64_t c8) {
  const uint64_t x = w ^ c8;
  const uint64_t lo7 = 0x7F7F7F7F7F7F7F7Full;
  return ~(((x & lo7) + lo7) | x | lo7);
}

// The thread's 64 bytes at t + off: 0x80 per '\n' (mn) and per token start (mk), for the bytes below len only.
__device__ __forceinline__ void chunk_masks(const char* __restrict__ t, int64_t len, int64_t off, uint64_t (&mn)[8], uint64_t (&mk)[8],
                                            int& n_nl, int& n_tok) {
  uint64_t w[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ulonglong2 v = {0ull, 0ull};
    if (off + 16 * q < len) v = *reinterpret_cast<const ulonglong2*>(t + off + 16 * q);  // the buffer holds len + 64 bytes
    w[2 * q] = v.x;
    w[2 * q + 1] = v.y;
  }
  // the byte before the chunk: a piece starts at the text's start or after a separator
  uint64_t prev = (off > 0 && off <= len && !mt::is_sep(t[off - 1])) ? 0x80ull : 0ull;
  n_nl = 0;
  n_tok = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t wo = off + 8 * q;
    uint64_t valid = 0x8080808080808080ull;
    if (wo + 8 > len) valid = wo >= len ? 0ull : (valid >> (8 * (8 - (int)(len - wo))));
    const uint64_t nl = eq_bytes(w[q], 0x0A0A0A0A0A0A0A0Aull);
    const uint64_t sep = nl | eq_bytes(w[q], 0x2020202020202020ull);
    const uint64_t tok = ~sep & valid;           // bytes of tokens
    const uint64_t before = (tok << 8) | prev;   // ... whose predecessor is a token byte too
    mn[q] = nl & valid;
    mk[q] = tok & ~before;
    prev = tok >> 56;
    n_nl += __popcll(mn[q]);
    n_tok += __popcll(mk[q]);
  }
}

__global__ __launch_bounds__(kBlock) void k_mt_counts(const char* __restrict__ t, int64_t len, int64_t n_tiles,
                                                      int64_t* __restrict__ cnt_nl, int64_t* __restrict__ cnt_tok) {
  __shared__ int red[2][kWavesPerBlock];
  for (int64_t tile = blockIdx.x; tile <= n_tiles; tile += gridDim.x) {
    if (tile == n_tiles) {  // the word the exclusive scans turn into the totals
      if (threadIdx.x == 0) cnt_nl[tile] = cnt_tok[tile] = 0;
      continue;
    }
    const int64_t off = tile * kMtTile + (int64_t)threadIdx.x * kMtChunk;
    uint64_t mn[8], mk[8];
    int nl, tk;
    chunk_masks(t, len, off, mn, mk, nl, tk);
    for (int s = 1; s < kWave; s <<= 1) {
      nl += __shfl_xor(nl, s, kWave);
      tk += __shfl_xor(tk, s, kWave);
    }
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) {
      red[0][threadIdx.x >> 6] = nl;
      red[1][threadIdx.x >> 6] = tk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int a = 0, b = 0;
      for (int v = 0; v < kWavesPerBlock; ++v) {
        a += red[0][v];
        b += red[1][v];
      }
      cnt_nl[tile] = a;
      cnt_tok[tile] = b;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_mt_positions(const char* __restrict__ t, int64_t len, int64_t n_tiles,
                                                         const int64_t* __restrict__ off_nl, const int64_t* __restrict__ off_tok,
                                                         int32_t* __restrict__ pos_nl, int64_t cap_nl, int32_t* __restrict__ pos_tok,
                                                         int64_t cap_tok) {
  __shared__ int scan[2][kBlock];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t off = tile * kMtTile + (int64_t)threadIdx.x * kMtChunk;
    uint64_t mn[8], mk[8];
    int nl, tk;
    chunk_masks(t, len, off, mn, mk, nl, tk);
    __syncthreads();
    scan[0][threadIdx.x] = nl;
    scan[1][threadIdx.x] = tk;
    __syncthreads();
    for (int s = 1; s < kBlock; s <<= 1) {  // inclusive scan over the workgroup's threads
      int a = 0, b = 0;
      if ((int)threadIdx.x >= s) {
        a = scan[0][threadIdx.x - s];
        b = scan[1][threadIdx.x - s];
      }
      __syncthreads();
      scan[0][threadIdx.x] += a;
      scan[1][threadIdx.x] += b;
      __syncthreads();
    }
    int64_t on = off_nl[tile] + scan[0][threadIdx.x] - nl, ot = off_tok[tile] + scan[1][threadIdx.x] - tk;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint64_t m = mn[q];
      while (m) {
        const int b = (__ffsll((long long)m) - 1) >> 3;
        if (on < cap_nl) pos_nl[on] = (int32_t)(off + 8 * q + b);
        ++on;
        m &= m - 1;
      }
      m = mk[q];
      while (m) {
        const int b = (__ffsll((long long)m) - 1) >> 3;
        if (ot < cap_tok) pos_tok[ot] = (int32_t)(off + 8 * q + b);
        ++ot;
        m &= m - 1;
      }
    }
  }
}

// first index whose value is not below v
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// thread j < n_nl: the line that the piece's j-th '\n' ends; thread n_nl: the open line at the piece's end and the carry
__global__ __launch_bounds__(kBlock) void k_mt_lines(const int64_t* __restrict__ tot_nl, const int64_t* __restrict__ tot_tok,
                                                     const int32_t* __restrict__ pos_nl, int64_t cap_nl,
                                                     const int32_t* __restrict__ pos_tok, int64_t cap_tok, int64_t row0, int64_t n_rows,
                                                     int64_t row_len, int last_open, const mt::Carry* __restrict__ carry_in,
                                                     mt::Carry* __restrict__ carry_out, long long* __restrict__ st) {
  const int64_t n_nl = min64(*tot_nl, cap_nl), n_tok = min64(*tot_tok, cap_tok);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= n_nl; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t first = j ? lower_bound_i32(pos_tok, n_tok, (int64_t)pos_nl[j - 1] + 1) : 0;
    const int64_t end = j < n_nl ? lower_bound_i32(pos_tok, n_tok, pos_nl[j]) : n_tok;
    const int64_t tokens = end - first + (j == 0 ? carry_in->col : 0);
    if (j < n_nl) {
      if (mt::line_is_short(tokens, row_len)) atomicAdd((unsigned long long*)&st[ST_BAD], 1ull);
      continue;
    }
    if (last_open && mt::line_is_short(tokens, row_len)) atomicAdd((unsigned long long*)&st[ST_BAD], 1ull);
    const int64_t row = row0 + n_nl;
    carry_out->col = tokens;
    carry_out->next = row < n_rows ? row * row_len + min64(tokens, row_len) : n_rows * row_len;
  }
}

// one thread per token of the piece t[0, len), which starts at byte `base` of the call's text
__global__ __launch_bounds__(kBlock) void k_mt_parse(const char* __restrict__ t, int64_t len, int64_t base,
                                                     const int64_t* __restrict__ tot_nl, const int64_t* __restrict__ tot_tok,
                                                     const int32_t* __restrict__ pos_nl, int64_t cap_nl,
                                                     const int32_t* __restrict__ pos_tok, int64_t cap_tok, int64_t row0, int64_t n_rows,
                                                     int64_t row_len, const mt::Carry* __restrict__ carry_in,
                                                     const Pow5* __restrict__ table, double* __restrict__ values,
                                                     long long* __restrict__ st, MtFix* __restrict__ fix) {
  const int64_t n_nl = min64(*tot_nl, cap_nl), n_tok = min64(*tot_tok, cap_tok);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_tok; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pos = pos_tok[i];
    if (pos < 0 || pos >= len) continue;
    const int64_t line = lower_bound_i32(pos_nl, n_nl, pos);  // '\n' before the token
    const int64_t first = line ? lower_bound_i32(pos_tok, n_tok, (int64_t)pos_nl[line - 1] + 1) : 0;
    const int64_t row = row0 + line, col = i - first + (line == 0 ? carry_in->col : 0);
    int64_t e = pos;
    while (e < len && e - pos <= mt::kMaxToken && !mt::is_sep(t[e])) ++e;
    double v = 0.0;
    int fl = 0;
    if (!mt::token_value(t + pos, e - pos, &v, &fl, table)) {
      atomicAdd((unsigned long long*)&st[ST_BAD], 1ull);
      continue;
    }
    if (col >= row_len || row >= n_rows) continue;  // read as float() reads it, then dropped as [:row_len] drops it
    const int64_t slot = row * row_len + col;
    values[slot] = v;
    if (fl & num::kNeedsStrtod) {
      const unsigned long long k = atomicAdd((unsigned long long*)&st[ST_FIX], 1ull);
      if (k < (unsigned long long)kMtMaxFix) fix[k] = MtFix{base + pos, slot};
    }
  }
}

unsigned grid_for(int64_t n, int per = kBlock) {
  int64_t b = (n + per - 1) / per;
  if (b > kMtGridCap) b = kMtGridCap;
  return (unsigned)(b < 1 ? 1 : b);
}

#define MT_LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__)

}  // namespace

int parse_f64_text(nfm_ctx* ctx, const char* text, int64_t len, int64_t n_rows, int64_t row_len, int64_t chunk_bytes, double* values,
                   int64_t* consumed, int32_t* clean, TextStats* stats) {
  hipStream_t st = ctx->stream;
  const double t_begin = dump_now_ms();
  *consumed = 0;
  *clean = 1;
  if (stats) *stats = TextStats();
  if (n_rows == 0) return NFM_OK;
  const int64_t count = n_rows * row_len;
  const int64_t chunk = mt::chunk_of(chunk_bytes);
  mt::Piece cur = mt::next_piece(text, len, 0, 0, n_rows, chunk);
  if (!cur.ok) {
    *clean = 0;
    return NFM_OK;
  }
  // the longest piece: the first one when it is the only one, else what a chunk can hold
  const int64_t piece_cap = cur.last ? cur.end - cur.begin : std::min(chunk, len);
  const int64_t max_tiles = (piece_cap + kMtTile - 1) / kMtTile;
  const int64_t cap_tok = piece_cap / 2 + 1;  // a token and the separator after it take two bytes at least

  DevBuf table, vals, status, fix, carry, cnt_nl, cnt_tok, off_nl, off_tok, pos_nl, pos_tok, scan_tmp;
  DumpPipe P;  // destroyed first: both streams are drained before the blocks above go back to the cache
  P.ctx = ctx;
  NFM_TRY(upload_pow5_table(ctx, &table));
  NFM_TRY(vals.alloc(sizeof(double) * std::max<int64_t>(count, 1)));
  NFM_TRY(status.alloc(sizeof(long long) * ST_COUNT));
  NFM_TRY(fix.alloc(sizeof(MtFix) * kMtMaxFix));
  NFM_TRY(carry.alloc(sizeof(mt::Carry) * 2));
  NFM_HIP_CHECK(hipMemsetAsync(status.p, 0, sizeof(long long) * ST_COUNT, st));
  NFM_HIP_CHECK(hipMemsetAsync(carry.p, 0, sizeof(mt::Carry) * 2, st));
  NFM_TRY(cnt_nl.alloc(sizeof(int64_t) * (max_tiles + 1)));
  NFM_TRY(cnt_tok.alloc(sizeof(int64_t) * (max_tiles + 1)));
  NFM_TRY(off_nl.alloc(sizeof(int64_t) * (max_tiles + 1)));
  NFM_TRY(off_tok.alloc(sizeof(int64_t) * (max_tiles + 1)));
  NFM_TRY(pos_tok.alloc(sizeof(int32_t) * cap_tok));
  size_t scan_bytes = 0;
  NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int)(max_tiles + 1), st));
  NFM_TRY(scan_tmp.alloc(scan_bytes ? scan_bytes : 1));
  NFM_TRY(P.open(ctx, TextSink(), piece_cap + 64, false));

  double stage_ms = 0.0;
  int64_t v_done = 0, n_pieces = 0;
  bool bad = false;
  // piece p - 1 has been queued on slot O: wait for its parse, then copy its values back beside the parse of piece p
  auto retire = [&](DumpPipe::Slot& O) -> int {
    if (!O.busy) return NFM_OK;
    O.busy = false;
    NFM_HIP_CHECK(hipEventSynchronize(O.fmt));
    float ms = 0.0f;
    NFM_HIP_CHECK(hipEventElapsedTime(&ms, O.c0, O.c1));
    P.copy_ms += ms;
    if (O.tot[2] != 0) {
      bad = true;
      return NFM_OK;
    }
    const int64_t v_next = std::min(std::max(O.tot[1], v_done), count);
    if (v_next > v_done) {
      const double t0 = dump_now_ms();
      NFM_HIP_CHECK(hipMemcpyAsync(values + v_done, vals.as<double>() + v_done, sizeof(double) * (size_t)(v_next - v_done),
                                   hipMemcpyDeviceToHost, P.copy_stream));
      NFM_HIP_CHECK(hipStreamSynchronize(P.copy_stream));
      P.copy_ms += dump_now_ms() - t0;
    }
    v_done = v_next;
    return NFM_OK;
  };

  for (int64_t p = 0;; ++p) {
    DumpPipe::Slot& S = P.slot[p & 1];
    const int64_t plen = cur.end - cur.begin;
    const int64_t n_tiles = (plen + kMtTile - 1) / kMtTile;
    NFM_CHECK(plen <= piece_cap && n_tiles <= max_tiles, NFM_ERR_HIP, "a piece of %lld bytes where at most %lld fit", (long long)plen,
              (long long)piece_cap);
    // the slot's last piece (p - 2) was retired in the round before: its text buffers are free
    const double t0 = dump_now_ms();
    memcpy(S.pin, text + cur.begin, (size_t)plen);
    stage_ms += dump_now_ms() - t0;
    NFM_HIP_CHECK(hipEventRecord(S.c0, P.copy_stream));
    if (plen) NFM_HIP_CHECK(hipMemcpyAsync(S.out.p, S.pin, (size_t)plen, hipMemcpyHostToDevice, P.copy_stream));
    NFM_HIP_CHECK(hipEventRecord(S.c1, P.copy_stream));
    NFM_HIP_CHECK(hipStreamWaitEvent(st, S.c1, 0));
    const int64_t cap_nl = std::max<int64_t>(cur.n_nl, 1);
    if (!pos_nl.p || pos_nl.bytes < sizeof(int32_t) * cap_nl) {  // grows only: the kernels of the piece before may still read it
      NFM_HIP_CHECK(hipStreamSynchronize(st));
      NFM_TRY(pos_nl.alloc(sizeof(int32_t) * cap_nl));
    }
    const char* t = S.out.as<char>();
    const mt::Carry* c_in = carry.as<mt::Carry>() + (p & 1);
    mt::Carry* c_out = carry.as<mt::Carry>() + ((p & 1) ^ 1);
    const int64_t* tot_nl = off_nl.as<int64_t>() + n_tiles;
    const int64_t* tot_tok = off_tok.as<int64_t>() + n_tiles;
    {
      TimedLaunch tl(ctx, "load_index");
      MT_LAUNCH(k_mt_counts, grid_for(n_tiles + 1, 1), t, plen, n_tiles, cnt_nl.as<int64_t>(), cnt_tok.as<int64_t>());
      size_t b = scan_bytes;
      NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scan_tmp.p, b, cnt_nl.as<int64_t>(), off_nl.as<int64_t>(), (int)(n_tiles + 1), st));
      b = scan_bytes;
      NFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scan_tmp.p, b, cnt_tok.as<int64_t>(), off_tok.as<int64_t>(), (int)(n_tiles + 1), st));
      if (n_tiles)
        MT_LAUNCH(k_mt_positions, grid_for(n_tiles, 1), t, plen, n_tiles, off_nl.as<int64_t>(), off_tok.as<int64_t>(),
                  pos_nl.as<int32_t>(), cap_nl, pos_tok.as<int32_t>(), cap_tok);
    }
    NFM_HIP_CHECK(hipGetLastError());
    {
      TimedLaunch tl(ctx, "load_parse");
      MT_LAUNCH(k_mt_lines, grid_for(cur.n_nl + 1), tot_nl, tot_tok, pos_nl.as<int32_t>(), cap_nl, pos_tok.as<int32_t>(), cap_tok,
                cur.row0, n_rows, row_len, cur.last && cur.open_line ? 1 : 0, c_in, c_out, status.as<long long>());
      MT_LAUNCH(k_mt_parse, grid_for(plen / 8 + 1), t, plen, cur.begin, tot_nl, tot_tok, pos_nl.as<int32_t>(), cap_nl,
                pos_tok.as<int32_t>(), cap_tok, cur.row0, n_rows, row_len, c_in, table.as<Pow5>(), vals.as<double>(),
                status.as<long long>(), fix.as<MtFix>());
    }
    NFM_HIP_CHECK(hipGetLastError());
    NFM_HIP_CHECK(hipMemcpyAsync(&S.tot[0], c_out, sizeof(mt::Carry), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipMemcpyAsync(&S.tot[2], status.p, sizeof(long long) * ST_COUNT, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipEventRecord(S.fmt, st));
    S.busy = true;
    ++n_pieces;
    NFM_TRY(retire(P.slot[(p & 1) ^ 1]));
    if (bad || cur.last) break;
    cur = mt::next_piece(text, len, cur.end, cur.row0 + cur.n_nl, n_rows, chunk);
    if (!cur.ok) {
      bad = true;
      break;
    }
  }
  NFM_TRY(retire(P.slot[0]));
  NFM_TRY(retire(P.slot[1]));
  if (stats) {
    stats->pieces = n_pieces;
    stats->bytes = cur.end;
    stats->copy_ms = P.copy_ms;
    stats->sink_ms = stage_ms;
  }
  if (bad) {
    *clean = 0;
    if (stats) stats->total_ms = dump_now_ms() - t_begin;
    return NFM_OK;
  }
  NFM_CHECK(v_done == count, NFM_ERR_HIP, "a clean block of %lld values gave %lld", (long long)count, (long long)v_done);
  // tokens for strtod (rare): re-read from the host's text.  The status words were copied after the last piece's kernels.
  long long h_st[ST_COUNT] = {0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(h_st, status.p, sizeof(h_st), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  if (h_st[ST_BAD] != 0 || h_st[ST_FIX] > kMtMaxFix) {
    *clean = 0;
  } else if (h_st[ST_FIX] > 0) {
    std::vector<MtFix> fx((size_t)h_st[ST_FIX]);
    NFM_HIP_CHECK(hipMemcpyAsync(fx.data(), fix.p, sizeof(MtFix) * fx.size(), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    std::string tok;
    for (const MtFix& r : fx) {
      if (r.pos < 0 || r.pos >= cur.end || r.slot < 0 || r.slot >= count) continue;
      int64_t e = r.pos;
      while (e < cur.end && !mt::is_sep(text[e])) ++e;
      tok.assign(text + r.pos, (size_t)(e - r.pos));
      values[r.slot] = strtod(tok.c_str(), nullptr);
    }
  }
  *consumed = cur.end;
  if (stats) stats->total_ms = dump_now_ms() - t_begin;
  return NFM_OK;
}

}  // namespace nfm
