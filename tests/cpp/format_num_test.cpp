// Host build of nimfm_amd/csrc/format_num.h for tests/test_format_num.py.
//   format_num_test        : per stdin line a binary64 bit pattern in hex -> "<token> <bits of parse_float(token) in hex>"
//   format_num_test uint   : per stdin line an unsigned decimal integer -> format_uint's text
// Every token is also sized with format_float_length and taken through pack_dec / unpack_dec, as the dump kernels do it;
// a disagreement ends the program with status 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../nimfm_amd/csrc/format_num.h"

using namespace nfm::num;

static const Pow kFmt[] = NFM_FMT_POW5_TABLE_INIT;
static const Pow5 kPow5[] = NFM_POW5_TABLE_INIT;

int main(int argc, char** argv) {
  static_assert(sizeof(kFmt) / sizeof(kFmt[0]) == NFM_FMT_N_INV + NFM_FMT_N_POW, "table size");
  const bool uint_mode = argc > 1 && strcmp(argv[1], "uint") == 0;
  char line[128];
  char* tok = (char*)malloc(kFmtMaxFloat);  // exactly the documented room: the sanitizer build sees an overrun
  char* tok2 = (char*)malloc(kFmtMaxFloat);
  while (fgets(line, sizeof line, stdin)) {
    if (uint_mode) {
      const int n = format_uint(strtoull(line, nullptr, 10), tok);
      printf("%.*s\n", n, tok);
      continue;
    }
    union {
      uint64_t u;
      double d;
    } c, back;
    c.u = strtoull(line, nullptr, 16);
    const int n = format_float(c.d, tok, kFmt);
    uint64_t bits;
    int16_t ex;
    pack_dec(decompose(c.d, kFmt), &bits, &ex);
    const Dec d = unpack_dec(bits, ex);
    if (n > kFmtMaxFloat || format_float_length(c.d, kFmt) != n || dec_length(d) != n || dec_write(d, tok2) != n ||
        memcmp(tok, tok2, (size_t)n) != 0) {
      fprintf(stderr, "length / packed form disagree for %016llx\n", (unsigned long long)c.u);
      return 2;
    }
    int flags = 0;
    back.d = 0.0;
    const int used = parse_float(tok, n, &back.d, &flags, kPow5);
    if (used != n || flags) {
      fprintf(stderr, "parse_float read %d of %d characters (flags %d) for %016llx\n", used, n, flags, (unsigned long long)c.u);
      return 2;
    }
    printf("%.*s %016llx\n", n, tok, (unsigned long long)back.u);
  }
  free(tok);
  free(tok2);
  return 0;
}
