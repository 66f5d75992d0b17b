// tests/cpp/stream_pieces_test.cpp -- nimfm_amd/csrc/stream_pieces.h is plain C++: this builds with g++ alone (no HIP, no
// library).  Reads one case per line on stdin -- "esize chunk_bytes n count_0 ... count_{n-1}" -- and prints the header's
// answer: "chunk max_bytes total_bytes | cut_0 cut_1 ...".  Inside the program every answer is held to what a launch needs:
// the cuts ascend from 0 to n, a piece has a record at least, its bytes are what stream_span_bytes says, and a piece of more
// than one record stays within the chunk.  tests/test_cpp_stream_pieces.py compares the output with a plain restatement.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nimfm_amd/csrc/stream_pieces.h"

int main() {
  std::string line;
  long cases = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int esize = 0;
    int64_t chunk = 0, n = 0;
    in >> esize >> chunk >> n;
    std::vector<int64_t> indptr((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
      int64_t c = 0;
      in >> c;
      indptr[(size_t)r + 1] = indptr[(size_t)r] + c;
    }
    if (!in) {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    const nfm::StreamPieces P = nfm::stream_pieces(indptr.data(), n, esize, chunk);
    bool ok = !P.cut.empty() && P.cut.front() == 0 && P.cut.back() == n && P.chunk == nfm::stream_chunk(chunk);
    int64_t total = 0, longest = 0;
    for (int64_t p = 0; ok && p < P.n_pieces(); ++p) {
      const int64_t r0 = P.cut[(size_t)p], r1 = P.cut[(size_t)p + 1];
      const int64_t bytes = nfm::stream_span_bytes(indptr.data(), r0, r1, esize);
      ok = r1 > r0 && (r1 - r0 == 1 || bytes <= P.chunk);
      // greedy: the next record would not have fitted
      if (ok && r1 < n) ok = bytes + nfm::stream_record_bytes(indptr.data(), r1, esize) > P.chunk;
      total += bytes;
      if (bytes > longest) longest = bytes;
    }
    ok = ok && total == P.total_bytes && longest == P.max_bytes && total == 8 * n + (int64_t)esize * indptr[(size_t)n];
    if (!ok) {
      std::fprintf(stderr, "PROPERTY VIOLATED: %s\n", line.c_str());
      return 1;
    }
    std::printf("%lld %lld %lld |", (long long)P.chunk, (long long)P.max_bytes, (long long)P.total_bytes);
    for (int64_t c : P.cut) std::printf(" %lld", (long long)c);
    std::printf("\n");
    ++cases;
  }
  std::fprintf(stderr, "%ld cases\n", cases);
  return 0;
}
