/* tools/cd_cpu.c -- the CPU yardstick of tools/cd_time.py: one thread, a C restatement of the reference's coordinate
 * descent for a degree-2 FM with squared loss (optimizer/cd.nim epochDeg2 :77-107, fit_linear.nim fitLinearCD / fitInterceptCD),
 * over a column-major copy of the data, in the reference's loop order.  Built with -O2 -ffp-contract=off.
 * Input file: int64 n, d, nnz, k, epochs; int64 indptr[n+1]; int64 indices[nnz]; double data[nnz]; double y[n].
 * Prints: "<ms per epoch> <final mean loss>". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double now_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hdr[5];
  if (fread(hdr, sizeof(int64_t), 5, f) != 5) return 2;
  const int64_t n = hdr[0], d = hdr[1], nnz = hdr[2], k = hdr[3], epochs = hdr[4];
  int64_t* rp = malloc(sizeof(int64_t) * (n + 1));
  int64_t* ri = malloc(sizeof(int64_t) * nnz);
  double* rv = malloc(sizeof(double) * nnz);
  double* y = malloc(sizeof(double) * n);
  if (fread(rp, sizeof(int64_t), n + 1, f) != (size_t)(n + 1) || fread(ri, sizeof(int64_t), nnz, f) != (size_t)nnz ||
      fread(rv, sizeof(double), nnz, f) != (size_t)nnz || fread(y, sizeof(double), n, f) != (size_t)n)
    return 2;
  fclose(f);
  /* the column twin, sample ids ascending */
  int64_t* cp = calloc(d + 1, sizeof(int64_t));
  for (int64_t q = 0; q < nnz; ++q) cp[ri[q] + 1]++;
  for (int64_t j = 0; j < d; ++j) cp[j + 1] += cp[j];
  int64_t* at = malloc(sizeof(int64_t) * d);
  memcpy(at, cp, sizeof(int64_t) * d);
  int64_t* cr = malloc(sizeof(int64_t) * nnz);
  double* cv = malloc(sizeof(double) * nnz);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t q = rp[i]; q < rp[i + 1]; ++q) {
      const int64_t pos = at[ri[q]]++;
      cr[pos] = i;
      cv[pos] = rv[q];
    }
  const double alpha0 = 1e-7 * n, alpha = 1e-5 * n, beta = 1e-3 * n;
  double* P = malloc(sizeof(double) * k * d);
  double* w = calloc(d, sizeof(double));
  double b = 0.0;
  srand(1);
  for (int64_t t = 0; t < k * d; ++t) P[t] = 0.01 * ((double)rand() / RAND_MAX - 0.5);
  double* colsq = calloc(d, sizeof(double));
  for (int64_t j = 0; j < d; ++j) {
    double s = 0.0;
    for (int64_t q = cp[j]; q < cp[j + 1]; ++q) s += cv[q] * cv[q];
    const double r = pow(s, 0.5);
    colsq[j] = r * r;
  }
  double* yp = calloc(n, sizeof(double));
  double* cache = calloc(n, sizeof(double));
  for (int64_t s = 0; s < k; ++s) { /* yPred: anova of degree 2 per component */
    double* a1 = calloc(n, sizeof(double));
    double* a2 = calloc(n, sizeof(double));
    for (int64_t j = 0; j < d; ++j)
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) {
        const double t = P[s * d + j] * cv[q];
        a1[cr[q]] += t;
        a2[cr[q]] += t * t;
      }
    for (int64_t i = 0; i < n; ++i) yp[i] += (a1[i] * a1[i] - a2[i]) / 2.0;
    free(a1);
    free(a2);
  }
  const double t0 = now_ms();
  for (int64_t e = 0; e < epochs; ++e) {
    double r = alpha0 * b; /* fitInterceptCD */
    for (int64_t i = 0; i < n; ++i) r += yp[i] - y[i];
    r /= (double)n + alpha0;
    b -= r;
    for (int64_t i = 0; i < n; ++i) yp[i] -= r;
    for (int64_t j = 0; j < d; ++j) { /* fitLinearCD */
      double u = alpha * w[j];
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) u += (yp[cr[q]] - y[cr[q]]) * cv[q];
      const double inv = colsq[j] + alpha;
      if (inv < 1e-12) continue;
      u /= inv;
      w[j] -= u;
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) yp[cr[q]] -= u * cv[q];
    }
    for (int64_t s = 0; s < k; ++s) { /* epochDeg2 */
      double* Ps = P + s * d;
      memset(cache, 0, sizeof(double) * n);
      for (int64_t j = 0; j < d; ++j)
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q) cache[cr[q]] += cv[q] * Ps[j];
      for (int64_t j = 0; j < d; ++j) {
        const double psj = Ps[j];
        double u = beta * psj, inv = 0.0;
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q) {
          const double dA = (cache[cr[q]] - psj * cv[q]) * cv[q];
          u += (yp[cr[q]] - y[cr[q]]) * dA;
          inv += dA * dA;
        }
        inv = inv + beta;
        if (inv < 1e-12) continue;
        u /= inv;
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q) {
          yp[cr[q]] -= u * (cache[cr[q]] - psj * cv[q]) * cv[q];
          cache[cr[q]] -= u * cv[q];
        }
        Ps[j] -= u;
      }
    }
  }
  const double ms = (now_ms() - t0) / (double)epochs;
  double loss = 0.0;
  for (int64_t i = 0; i < n; ++i) loss += 0.5 * (y[i] - yp[i]) * (y[i] - yp[i]);
  printf("%.6f %.10g\n", ms, loss / n);
  return 0;
}
