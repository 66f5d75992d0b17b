// nimfm_amd/csrc/model_text_pieces.h -- the decisions of nfm_parse_f64 that are not arithmetic: what
// a token is, where the text of a number block may be cut into pieces, what is carried across a cut, and when a text is
// "clean".  Free of HIP: g++ compiles it alone (tests/cpp/model_text_pieces_test.cpp), in the manner of stream_pieces.h and
// the route headers; model_text.hip's kernels use the same functions on the device.
//
// The text is the body of a "lams:", "P[o]:", "P:" or "w:" block of a model dump (model/factorization_machine.nim:142-165):
// n_rows lines of row_len numbers.  A TOKEN is a maximal run of bytes other than ' ' and '\n'; its row is the number of '\n'
// before it, its column its rank among the tokens of its line.  The block ends with its n_rows-th '\n', or with the text
// when the n_rows-th line has no '\n'.  A text is CLEAN when it has n_rows lines, every one of them has at least row_len
// tokens, and parse_float (parse_num.h) consumes every token of the block to its last byte -- the tokens beyond row_len
// too: the Python host calls float() on them before it drops them -- and no token is longer than kMaxToken bytes (what one
// device thread reads).  Anything else is left to the caller's own parser.
#pragma once
#include <stdint.h>
#include <string.h>

#include "parse_num.h"

namespace nfm {
namespace mt {

constexpr int64_t kDefaultChunk = (int64_t)128 << 20;  // as the dumps
constexpr int64_t kMaxChunk = (int64_t)1 << 30;        // positions inside a piece are int32
constexpr int64_t kMinChunk = 2;
constexpr int64_t kMaxToken = 1024;

NFM_HD bool is_sep(char c) { return c == ' ' || c == '\n'; }

inline int64_t chunk_of(int64_t chunk_bytes) {
  if (chunk_bytes <= 0) return kDefaultChunk;
  if (chunk_bytes < kMinChunk) return kMinChunk;
  return chunk_bytes < kMaxChunk ? chunk_bytes : kMaxChunk;
}

// One piece of the text [pos, len): where it ends, and what the host knows about it without reading a number.
struct Piece {
  int64_t begin = 0, end = 0;  // bytes [begin, end)
  int64_t row0 = 0;            // '\n' before `begin`, counted from the start of the block
  int64_t n_nl = 0;            // '\n' inside the piece
  bool last = false;           // the block ends with this piece
  bool open_line = false;      // last only: the final line has no '\n' (it ends with the text)
  bool ok = true;              // false: no cut is possible (a token longer than the chunk) or the text has too few lines
};

// The piece that starts at `pos`, where rows_done lines are complete.  It takes at most `chunk` bytes and ends
//   - right after the n_rows-th '\n' when that lies inside (the block's last piece), else
//   - with the text when what is left fits (the last piece: the n_rows-th line is then the unterminated one), else
//   - right after the last separator inside the chunk, so that no token spans two pieces.
// `pos` is therefore always the start of the text or the byte after a separator.
inline Piece next_piece(const char* text, int64_t len, int64_t pos, int64_t rows_done, int64_t n_rows, int64_t chunk) {
  Piece p;
  p.begin = pos;
  p.row0 = rows_done;
  int64_t e = len - pos <= chunk ? len : pos + chunk;
  int64_t q = pos;
  while (q < e) {  // the '\n' of the candidate span, up to the one that ends the block
    const void* hit = memchr(text + q, '\n', (size_t)(e - q));
    if (!hit) break;
    q = (const char*)hit - text + 1;
    ++p.n_nl;
    if (rows_done + p.n_nl == n_rows) {
      p.end = q;
      p.last = true;
      return p;
    }
  }
  if (e == len) {  // the text ends before the n_rows-th '\n'
    p.end = len;
    p.last = true;
    p.open_line = true;
    // the unterminated rest is the n_rows-th line only if it is the one line missing and is not empty
    p.ok = rows_done + p.n_nl == n_rows - 1 && len > 0 && text[len - 1] != '\n';
    return p;
  }
  int64_t c = e;  // cut back to the byte after the last separator
  while (c > pos && !is_sep(text[c - 1])) --c;
  if (c == pos) {
    p.ok = false;
    p.end = pos;
    return p;
  }
  p.end = c;  // the '\n' counted above all lie before c: the bytes cut off hold no separator
  return p;
}

// What is carried from piece to piece.  The row is the host's (it counts the '\n' to find the block's end); the column and
// the index of the next value are the device's, kept in device memory.
struct Carry {
  int64_t col = 0;     // tokens of the current (unterminated) line seen so far
  int64_t next = 0;    // values[0, next) are final: row * row_len + min(col, row_len)
};

// A line with `tokens` tokens has ended (by '\n', or by the end of the block's last, open line).
NFM_HD bool line_is_short(int64_t tokens, int64_t row_len) { return tokens < row_len; }

// The token text[0, n) -> value with the bits Python's float() gives.  false: not a number to its last byte.
// parse_float returns +nan for "-nan"; float() keeps the sign.
NFM_HD bool token_value(const char* s, int64_t n, double* out, int* flags, const num::Pow5* table) {
  double v = 0.0;
  if (n > kMaxToken) return false;
  const int used = num::parse_float(s, n, &v, flags, table);
  if (used <= 0 || used != n) return false;
  if (v != v && s[0] == '-') v = num::bits_to_double(0xFFF8ull << 48);
  *out = v;
  return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The serial walk of one piece: what the kernels of model_text.hip compute in parallel.  values may be written for a text
// that turns out not to be clean; *bad counts the reasons.  need_strtod(pos, slot) is called for a flagged token.
template <class Fix>
inline void walk_piece(const char* text, const Piece& p, int64_t n_rows, int64_t row_len, const num::Pow5* table, Carry* carry,
                       double* values, int64_t* bad, Fix&& need_strtod) {
  int64_t row = p.row0, col = carry->col;
  int64_t i = p.begin;
  while (i < p.end) {
    const char c = text[i];
    if (c == '\n') {
      if (line_is_short(col, row_len)) ++*bad;
      ++row;
      col = 0;
      ++i;
      continue;
    }
    if (c == ' ') {
      ++i;
      continue;
    }
    int64_t e = i;
    while (e < p.end && !is_sep(text[e])) ++e;
    double v = 0.0;
    int fl = 0;
    if (!token_value(text + i, e - i, &v, &fl, table)) {
      ++*bad;
    } else if (col < row_len && row < n_rows) {
      values[row * row_len + col] = v;
      if (fl & num::kNeedsStrtod) need_strtod(i, row * row_len + col);
    }
    ++col;
    i = e;
  }
  if (p.last && p.open_line && line_is_short(col, row_len)) ++*bad;
  carry->col = col;
  carry->next = row < n_rows ? row * row_len + (col < row_len ? col : row_len) : n_rows * row_len;
}
#endif

}  // namespace mt
}  // namespace nfm
