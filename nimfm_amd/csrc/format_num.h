// nimfm_amd/csrc/format_num.h -- number -> text for the dump kernels (dataset_text.hip), compiled for host and device
// from the same source: the mirror of parse_num.h.
//
// The reference writes a float64 with Nim's `$` (dataset.nim:793-805, 825-837; model/factorization_machine.nim:142-165),
// which this project spells as Python's repr (host.py::_nim_float, oracle/ingest.py): the SHORTEST decimal digit string
// that reads back to the same bits, the one nearest the value among the shortest, laid out
//   positional   when the decimal point position decpt satisfies -4 < decpt <= 16 ("1.0", "123456.0", "0.0001"), ".0"
//                appended to integral values,
//   exponent     otherwise: d[.ddd]e+XX / e-XX, at least two exponent digits, no ".0" ("1e+16", "1e-05", "5e-324"),
// "-0.0" keeps its sign, every NaN is "nan", the infinities are "inf" / "-inf".  The longest token has 24 characters
// ("-2.2250738585072014e-308").
//
// Digits: Ryu (U. Adams, "Ryu: Fast Float-to-String Conversion", PLDI 2018), the general loop with the exact
// trailing-zero bookkeeping, over the 125-bit tables of fmt_pow5_table.h.  Integer arithmetic only.
//
// A conversion is split in two so that a kernel can size a token in one pass and write it in another without the
// 128-bit products a second time: decompose() -> Dec (decimal significand, exponent, kind), then dec_length() /
// dec_write().  pack_dec / unpack_dec keep a Dec in ten bytes.
#pragma once
#include <stdint.h>

#include "fmt_pow5_table.h"
#include "parse_num.h"

namespace nfm {
namespace num {

typedef Pow5 Pow;  // {hi, lo}; format_float's table is NFM_FMT_POW5_TABLE_INIT

enum { kFmtMaxFloat = 24, kFmtMaxUint = 20 };
enum { DEC_FINITE = 0, DEC_INF = 1, DEC_NAN = 2, DEC_INT = 3 };  // DEC_INT: the digits of sig alone ("-1", not "-1.0")

struct Dec {
  uint64_t sig;  // decimal significand, below 10^17 (DEC_INT: any value below 2^57)
  int32_t exp;   // value = sig * 10^exp
  int32_t kind;
  bool neg;
};

// (m * t) >> j for j >= 64; the result fits 64 bits
NFM_HD uint64_t mul_shift(uint64_t m, const Pow t, int j) {
  uint64_t h0, l0, h2, l2;
  mul64(m, t.lo, h0, l0);
  mul64(m, t.hi, h2, l2);
  const uint64_t sl = h0 + l2;
  const uint64_t sh = h2 + (sl < h0 ? 1 : 0);
  const int d = j - 64;
  if (d == 0) return sl;
  if (d < 64) return (sh << (64 - d)) | (sl >> d);
  return sh >> (d - 64);
}

NFM_HD int pow5_bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }  // bit length of 5^e, e <= 3528
NFM_HD int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }       // floor(log10(2^e)), e <= 1650
NFM_HD int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }      // floor(log10(5^e)), e <= 2620

NFM_HD bool multiple_of_pow5(uint64_t v, int p) {  // v != 0
  int c = 0;
  while (c < p && v % 5 == 0) {
    v /= 5;
    ++c;
  }
  return c >= p;
}

NFM_HD int dec_digits(uint64_t v) {  // decimal digits of v (1 for 0)
  int n = 1;
  while (v >= 10000) {
    v /= 10000;
    n += 4;
  }
  return n + (v >= 1000 ? 3 : v >= 100 ? 2 : v >= 10 ? 1 : 0);
}

// shortest decimal of a finite non-zero binary64 given by its fields (Ryu's d2d)
NFM_HD void shortest_decimal(uint64_t ieee_m, int ieee_e, const Pow* table, uint64_t* sig, int32_t* exp10) {
  int e2;
  uint64_t m2;
  if (ieee_e == 0) {
    e2 = 1 - 1023 - 52 - 2;
    m2 = ieee_m;
  } else {
    e2 = ieee_e - 1023 - 52 - 2;
    m2 = (1ull << 52) | ieee_m;
  }
  const bool accept = (m2 & 1) == 0;
  const uint64_t mv = 4 * m2;
  const int mm_shift = (ieee_m != 0 || ieee_e <= 1) ? 1 : 0;
  uint64_t vr, vp, vm;
  int e10;
  bool vm_tz = false, vr_tz = false;
  if (e2 >= 0) {
    const int q = log10_pow2(e2) - (e2 > 3 ? 1 : 0);
    e10 = q;
    const int k = NFM_FMT_POW5_BITS + pow5_bits(q) - 1;
    const int j = -e2 + q + k;
    const Pow t = table[q];
    vr = mul_shift(mv, t, j);
    vp = mul_shift(mv + 2, t, j);
    vm = mul_shift(mv - 1 - mm_shift, t, j);
    if (q <= 21) {  // only then can mv * 2^e2 / 10^q be a multiple of 5^q: mv < 2^55 < 5^24
      if (mv % 5 == 0) vr_tz = multiple_of_pow5(mv, q);
      else if (accept) vm_tz = multiple_of_pow5(mv - 1 - mm_shift, q);
      else vp -= multiple_of_pow5(mv + 2, q) ? 1 : 0;
    }
  } else {
    const int q = log10_pow5(-e2) - (-e2 > 1 ? 1 : 0);
    e10 = q + e2;
    const int i = -e2 - q;
    const int k = pow5_bits(i) - NFM_FMT_POW5_BITS;
    const int j = q - k;
    const Pow t = table[NFM_FMT_N_INV + i];
    vr = mul_shift(mv, t, j);
    vp = mul_shift(mv + 2, t, j);
    vm = mul_shift(mv - 1 - mm_shift, t, j);
    if (q <= 1) {  // mv = 4 * m2 always has two trailing zero bits
      vr_tz = true;
      if (accept) vm_tz = mm_shift == 1;
      else --vp;
    } else if (q < 63) {
      vr_tz = (mv & ((1ull << q) - 1)) == 0;
    }
  }
  int removed = 0;
  int last = 0;
  uint64_t out;
  if (vm_tz || vr_tz) {  // rare
    while (vp / 10 > vm / 10) {
      vm_tz = vm_tz && vm % 10 == 0;
      vr_tz = vr_tz && last == 0;
      last = (int)(vr % 10);
      vr /= 10;
      vp /= 10;
      vm /= 10;
      ++removed;
    }
    if (vm_tz) {
      while (vm % 10 == 0) {
        vr_tz = vr_tz && last == 0;
        last = (int)(vr % 10);
        vr /= 10;
        vp /= 10;
        vm /= 10;
        ++removed;
      }
    }
    if (vr_tz && last == 5 && vr % 2 == 0) last = 4;  // exactly halfway: round to even
    out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5) ? 1 : 0);
  } else {
    bool up = false;
    while (vp / 10 > vm / 10) {
      up = vr % 10 >= 5;
      vr /= 10;
      vp /= 10;
      vm /= 10;
      ++removed;
    }
    out = vr + ((vr == vm || up) ? 1 : 0);
  }
  int32_t e = e10 + removed;
  while (out % 10 == 0) {  // out != 0; a rounded-up 9...9 leaves zeros behind
    out /= 10;
    ++e;
  }
  *sig = out;
  *exp10 = e;
}

NFM_HD Dec decompose(double v, const Pow* table) {
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  const uint64_t m = c.u & ((1ull << 52) - 1);
  const int e = (int)((c.u >> 52) & 0x7FF);
  Dec r;
  r.sig = 0;
  r.exp = 0;
  r.kind = DEC_FINITE;
  r.neg = (c.u >> 63) != 0;
  if (e == 0x7FF) {
    r.kind = m ? DEC_NAN : DEC_INF;
    if (m) r.neg = false;
  } else if (e != 0 || m != 0) {
    shortest_decimal(m, e, table, &r.sig, &r.exp);
  }
  return r;
}

NFM_HD Dec dec_from_int(int64_t v) {  // |v| below 2^57
  Dec r;
  r.neg = v < 0;
  r.sig = r.neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  r.exp = 0;
  r.kind = DEC_INT;
  return r;
}

// ten bytes: sig in bits 0..56, kind in bits 58..59, the sign in bit 63; the exponent beside it
NFM_HD void pack_dec(const Dec d, uint64_t* bits, int16_t* ex) {
  *bits = d.sig | ((uint64_t)d.kind << 58) | ((uint64_t)(d.neg ? 1 : 0) << 63);
  *ex = (int16_t)d.exp;
}
NFM_HD Dec unpack_dec(uint64_t bits, int16_t ex) {
  Dec d;
  d.sig = bits & ((1ull << 57) - 1);
  d.kind = (int32_t)((bits >> 58) & 3);
  d.neg = (bits >> 63) != 0;
  d.exp = ex;
  return d;
}

NFM_HD int dec_length(const Dec d) {
  const int s = d.neg ? 1 : 0;
  if (d.kind == DEC_NAN || d.kind == DEC_INF) return s + 3;
  if (d.kind == DEC_INT) return s + dec_digits(d.sig);
  if (d.sig == 0) return s + 3;
  const int n = dec_digits(d.sig), decpt = d.exp + n;
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) return s + 2 - decpt + n;
    if (decpt >= n) return s + decpt + 2;
    return s + n + 1;
  }
  const int ae = decpt - 1 < 0 ? 1 - decpt : decpt - 1;
  return s + n + (n > 1 ? 1 : 0) + 2 + (ae >= 100 ? 3 : 2);
}

NFM_HD void put_digits(char* p, uint64_t v, int n) {  // the low n digits of v, most significant first
  for (int i = n - 1; i >= 0; --i) {
    p[i] = (char)('0' + (int)(v % 10));
    v /= 10;
  }
}

NFM_HD uint64_t pow10_u64(int n) {  // n <= 19
  uint64_t p = 1;
  for (int i = 0; i < n; ++i) p *= 10;
  return p;
}

NFM_HD int dec_write(const Dec d, char* out) {
  char* p = out;
  if (d.neg) *p++ = '-';
  if (d.kind == DEC_NAN) {
    p[0] = 'n'; p[1] = 'a'; p[2] = 'n';
    return (int)(p - out) + 3;
  }
  if (d.kind == DEC_INF) {
    p[0] = 'i'; p[1] = 'n'; p[2] = 'f';
    return (int)(p - out) + 3;
  }
  if (d.kind == DEC_INT) {
    const int n = dec_digits(d.sig);
    put_digits(p, d.sig, n);
    return (int)(p - out) + n;
  }
  if (d.sig == 0) {
    p[0] = '0'; p[1] = '.'; p[2] = '0';
    return (int)(p - out) + 3;
  }
  const int n = dec_digits(d.sig), decpt = d.exp + n;
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) {
      *p++ = '0';
      *p++ = '.';
      for (int i = 0; i < -decpt; ++i) *p++ = '0';
      put_digits(p, d.sig, n);
      p += n;
    } else if (decpt >= n) {
      put_digits(p, d.sig, n);
      p += n;
      for (int i = n; i < decpt; ++i) *p++ = '0';
      *p++ = '.';
      *p++ = '0';
    } else {
      const uint64_t cut = pow10_u64(n - decpt);
      put_digits(p, d.sig / cut, decpt);
      p += decpt;
      *p++ = '.';
      put_digits(p, d.sig % cut, n - decpt);
      p += n - decpt;
    }
    return (int)(p - out);
  }
  if (n > 1) {
    const uint64_t cut = pow10_u64(n - 1);
    *p++ = (char)('0' + (int)(d.sig / cut));
    *p++ = '.';
    put_digits(p, d.sig % cut, n - 1);
    p += n - 1;
  } else {
    *p++ = (char)('0' + (int)d.sig);
  }
  int e = decpt - 1;
  *p++ = 'e';
  *p++ = e < 0 ? '-' : '+';
  if (e < 0) e = -e;
  const int ne = e >= 100 ? 3 : 2;
  put_digits(p, (uint64_t)e, ne);
  p += ne;
  return (int)(p - out);
}

// v as text at out (room for kFmtMaxFloat characters, no terminating NUL); returns the length
NFM_HD int format_float(double v, char* out, const Pow* table) { return dec_write(decompose(v, table), out); }
NFM_HD int format_float_length(double v, const Pow* table) { return dec_length(decompose(v, table)); }

// v in decimal at out (room for kFmtMaxUint characters); returns the length
NFM_HD int format_uint(uint64_t v, char* out) {
  const int n = dec_digits(v);
  put_digits(out, v, n);
  return n;
}

}  // namespace num
}  // namespace nfm
