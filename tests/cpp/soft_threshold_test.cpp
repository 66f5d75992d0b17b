// tests/cpp/soft_threshold_test.cpp -- the two spellings of softthreshold (regularizer/utils.nim:4-5) the device code has
// had agree bit for bit: the one nimfm_amd/csrc/prox_dev.h keeps, and the one cd.hip and pbcd.hip used to carry.  Host C++,
// built with -ffp-contract=off as the library is.  The edge values (signed zeros, NaN, infinities, |x| == a, denormals)
// crossed with each other, then random pairs: uniform in bits, and |x| close to a.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

static double kept(double x, double alpha) {  // prox_dev.h
  const double t = fmax(fabs(x) - alpha, 0.0);
  return x > 0 ? t : (x < 0 ? -t : 0.0 * t);
}
static double dropped(double x, double a) {  // cd.hip's soft_threshold, pbcd.hip's pb_soft
  const double m = fabs(x) - a;
  return (double)((x > 0.0) - (x < 0.0)) * (m > 0.0 ? m : 0.0);
}
static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof(u));
  return u;
}
static long bad = 0;
static void check(double x, double a) {
  const volatile double xv = x, av = a;  // no constant folding
  const double p = kept(xv, av), q = dropped(xv, av);
  if (bits(p) != bits(q) && bad++ < 20)
    std::printf("x = %a, a = %a: kept %a (%016llx), dropped %a (%016llx)\n", x, a, p, (unsigned long long)bits(p), q,
                (unsigned long long)bits(q));
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double dmin = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();
  const double edge[] = {0.0, -0.0, nan, -nan, inf, -inf, 1.0, -1.0, 1.5, -1.5, dmin, -dmin, 2.2250738585072014e-308,
                         -2.2250738585072014e-308, big, -big, 1.0 + 2.220446049250313e-16, 1.0 - 1.1102230246251565e-16,
                         -1.0 - 2.220446049250313e-16, 1e-300, -1e-300, 3.0, -3.0};
  long n = 0;
  for (double x : edge)
    for (double a : edge) {
      check(x, a);
      check(x, std::fabs(x));  // |x| == a
      check(x, -std::fabs(x));
      ++n;
    }
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> u(-4.0, 4.0);
  for (long i = 0; i < 1000000; ++i, ++n) {
    double x, a;
    const uint64_t bx = rng(), ba = rng();
    std::memcpy(&x, &bx, sizeof(x));  // any bit pattern: every exponent, NaNs with payloads, denormals
    std::memcpy(&a, &ba, sizeof(a));
    check(x, a);
  }
  for (long i = 0; i < 1000000; ++i, ++n) {
    const double x = u(rng), a = std::fabs(x) + (double)((int)(rng() % 5) - 2) * 2.220446049250313e-16 * std::fabs(x);
    check(x, a);       // |x| within two ulps of a
    check(x, u(rng));  // ordinary magnitudes
  }
  if (bad) {
    std::printf("soft threshold: %ld of %ld pairs differ\n", bad, n);
    return 1;
  }
  std::printf("soft threshold ok: %ld pairs\n", n);
  return 0;
}
