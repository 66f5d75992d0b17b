// nimfm_amd/csrc/stream_pieces.h -- where the body of a binary stream file (tensor/sparse_stream.nim:3-33) is cut into the
// pieces dataset_stream.hip packs one at a time.  Host-only and free of HIP: g++ compiles it alone
// (tests/cpp/stream_pieces_test.cpp), in the manner of mb_route.h / seq_route.h.
//
// Record r of the body is an int64 count and count elements of esize bytes (16: {val, id}; 24: {field, val, id}), so it
// takes 8 + esize * (indptr[r + 1] - indptr[r]) bytes.  The cuts are a pure function of indptr, esize and chunk_bytes:
// a piece takes records while its bytes stay within the chunk, and one record at least -- a record longer than the chunk is
// a piece by itself.
#pragma once
#include <stdint.h>

#include <vector>

namespace nfm {

constexpr int64_t kStreamDefaultChunk = (int64_t)128 << 20;  // as nfm_dataset_dump_svmlight
constexpr int64_t kStreamMaxChunk = (int64_t)1 << 30;

struct StreamPieces {
  std::vector<int64_t> cut;  // piece p holds the records [cut[p], cut[p + 1]); cut[0] = 0, cut.back() = n
  int64_t chunk = 0;         // the chunk size in force
  int64_t max_bytes = 0;     // of the longest piece
  int64_t total_bytes = 0;   // of the body
  int64_t n_pieces() const { return (int64_t)cut.size() - 1; }
};

inline int64_t stream_chunk(int64_t chunk_bytes) {
  if (chunk_bytes <= 0) return kStreamDefaultChunk;
  return chunk_bytes < kStreamMaxChunk ? chunk_bytes : kStreamMaxChunk;
}

inline int64_t stream_record_bytes(const int64_t* indptr, int64_t r, int esize) { return 8 + (int64_t)esize * (indptr[r + 1] - indptr[r]); }

// bytes of the records [r0, r1): they are contiguous in the body
inline int64_t stream_span_bytes(const int64_t* indptr, int64_t r0, int64_t r1, int esize) {
  return 8 * (r1 - r0) + (int64_t)esize * (indptr[r1] - indptr[r0]);
}

inline StreamPieces stream_pieces(const int64_t* indptr, int64_t n, int esize, int64_t chunk_bytes) {
  StreamPieces P;
  P.chunk = stream_chunk(chunk_bytes);
  P.cut.push_back(0);
  for (int64_t r = 0; r < n;) {
    int64_t bytes = 0, r1 = r;
    while (r1 < n) {
      const int64_t b = stream_record_bytes(indptr, r1, esize);
      if (r1 > r && bytes + b > P.chunk) break;
      bytes += b;
      ++r1;
    }
    if (bytes > P.max_bytes) P.max_bytes = bytes;
    P.total_bytes += bytes;
    P.cut.push_back(r1);
    r = r1;
  }
  return P;
}

}  // namespace nfm
