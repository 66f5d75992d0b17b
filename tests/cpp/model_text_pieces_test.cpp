// tests/cpp/model_text_pieces_test.cpp -- nimfm_amd/csrc/model_text_pieces.h without HIP: the cuts, the carry and the serial
// walk that the kernels of model_text.hip restate in parallel.  Reads cases on stdin, one after the other:
//   "n_rows row_len first_chunk chunk len\n" followed by len bytes of text
// (first_chunk > 0: the first piece is cut with that chunk size, the others with `chunk`), and prints per case
//   "clean consumed pieces fixes" and, when clean, the values' bits in hex on the next line.
// Tokens flagged kNeedsStrtod are re-read with strtod, as the host side of nfm_parse_f64 does.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../nimfm_amd/csrc/model_text_pieces.h"

using namespace nfm;

static const num::Pow5 kTable[] = NFM_POW5_TABLE_INIT;

int main() {
  long long n_rows, row_len, first_chunk, chunk_bytes, len;
  while (scanf("%lld %lld %lld %lld %lld", &n_rows, &row_len, &first_chunk, &chunk_bytes, &len) == 5) {
    if (getchar() != '\n') return 2;
    std::vector<char> text((size_t)len + 1);  // exactly len readable bytes matter: the sanitizer build checks the walk stays inside
    if (len && fread(text.data(), 1, (size_t)len, stdin) != (size_t)len) return 2;
    text.resize((size_t)len);
    text.shrink_to_fit();
    std::vector<double> values((size_t)(n_rows * row_len));
    struct Fix {
      int64_t pos, slot;
    };
    std::vector<Fix> fixes;
    int64_t bad = 0, pieces = 0, consumed = 0;
    bool clean = true;
    if (n_rows > 0) {
      mt::Carry carry;
      const int64_t chunk = mt::chunk_of(chunk_bytes);
      mt::Piece p = mt::next_piece(text.data(), len, 0, 0, n_rows, first_chunk > 0 ? mt::chunk_of(first_chunk) : chunk);
      for (;;) {
        if (!p.ok) {
          clean = false;
          break;
        }
        ++pieces;
        const int64_t next_before = carry.next;
        mt::walk_piece(text.data(), p, n_rows, row_len, kTable, &carry, values.data(), &bad,
                       [&](int64_t pos, int64_t slot) { fixes.push_back(Fix{pos, slot}); });
        if (bad == 0 && carry.next < next_before) return 3;  // the values of a piece follow those of the piece before
        consumed = p.end;
        if (p.last) break;
        p = mt::next_piece(text.data(), len, p.end, p.row0 + p.n_nl, n_rows, chunk);
      }
      if (bad) clean = false;
      if (clean && carry.next != n_rows * row_len) return 4;
    }
    if (clean) {
      for (const Fix& f : fixes) {
        int64_t e = f.pos;
        while (e < consumed && !mt::is_sep(text[(size_t)e])) ++e;
        const std::string tok(text.data() + f.pos, (size_t)(e - f.pos));
        values[(size_t)f.slot] = strtod(tok.c_str(), nullptr);
      }
    }
    printf("%d %lld %lld %zu\n", clean ? 1 : 0, (long long)(clean ? consumed : 0), (long long)pieces, fixes.size());
    if (clean) {
      for (double v : values) {
        unsigned long long b;
        memcpy(&b, &v, 8);
        printf("%016llx", b);
      }
      printf("\n");
    }
  }
  return 0;
}
