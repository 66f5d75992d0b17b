// nimfm_amd/csrc/cfm_dev.h -- what the device code of the two solvers of the convex factorization machine shares: cfm.hip
// (Hazan) and gcd.hip (GreedyCD, section 21).  The row / column pass helpers, the fixed-tree sums and
// the layout of HazanState::vec.  The kernels both solvers run (k_rows, k_cols, the power method) live in cfm.hip and are
// reached through the host functions of cfm.h.
#pragma once
#include "cd_dev.h"
#include "cfm.h"

namespace nfm {
namespace {

constexpr int kG = 8;                 // lanes per row / column
constexpr int kGroups = kBlock / kG;  // rows / columns per workgroup

inline int64_t blocks_for(int64_t n, int per) { return n <= 0 ? 1 : (n + per - 1) / per; }

struct Twin {
  const int64_t* rptr;
  const int32_t* ridx;
  const double* rval;
  const int64_t* cptr;
  const int32_t* crow;
  const double* cval;
  int64_t n, d;
};

// acc + f(q0) + f(q0 + 1) + ... in that order; the kG lanes of a group call it together (q0, q1 uniform in the group) and
// all return the same value.  `base` is the group's first lane in the wavefront.
template <class F>
__device__ __forceinline__ double ordered_acc(double acc, int64_t q0, int64_t q1, int gl, int base, F f) {
  for (int64_t c = q0; c < q1; c += kG) {
    const int64_t q = c + gl;
    const double t = q < q1 ? f(q) : 0.0;
#pragma unroll
    for (int u = 0; u < kG; ++u) {
      const double tu = dev::shfl_d(t, base + u);
      if (c + u < q1) acc += tu;
    }
  }
  return acc;
}

// K[s, i] of one basis vector Ps for the row [q0, q1): anova (kernels.nim:22-43) or poly (:67-79), degree 2; the kG lanes of
// a group call it together
__device__ __forceinline__ double kernel_value(const int32_t* ridx, const double* rval, const double* Ps, int64_t q0, int64_t q1, int gl, int base,
                                               int ignore_diag) {
  const double a1 = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return Ps[ridx[q]] * rval[q]; });
  if (!ignore_diag) return a1 * a1;
  const double a2 = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) {
    const double t = Ps[ridx[q]] * rval[q];
    return t * t;
  });
  return (a1 * a1 - a2) / 2.0;
}

// fixed tree over the first `width` slots of red (a power of two <= kBlock); every thread of the workgroup calls it
__device__ __forceinline__ double tree(double* red, int width) {
  __syncthreads();
  for (int s = width / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// second stage, in a workgroup of kNarrowBlock threads
__device__ __forceinline__ double fin_sum(const double* part, int64_t np, double* red) {
  double a = 0.0;
  for (int64_t t = threadIdx.x; t < np; t += kNarrowBlock) a += part[t];
  return block_sum(a, red);
}

// fixed tree over the kBlock elements of an element-wise workgroup
__device__ __forceinline__ double tree_block(double v, double* red) {
  red[threadIdx.x] = v;
  return tree(red, kBlock);
}

// the pieces of HazanState::vec.  GreedyCD keeps yPred in ypq, dL in res and colNormSq in cn; it leaves yt, ypl and the CG's
// vectors unused.
struct Lay {
  double *yt, *ypl, *ypq, *res, *Xp, *K, *pv, *q, *cn, *x, *b, *r, *cp, *Ap;
};
inline size_t pad32(size_t v) { return (v + 31) / 32 * 32; }
inline size_t lay_doubles(int64_t n, int64_t d, int maxc) { return pad32(n) * 5 + pad32((size_t)n * maxc) + pad32(d + 1) * 8; }
inline Lay layout(const HazanState* S) {
  Lay L;
  double* p = S->vec.as<double>();
  const size_t pn = pad32(S->n), pz = pad32(S->d + 1);
  L.yt = p; p += pn;
  L.ypl = p; p += pn;
  L.ypq = p; p += pn;
  L.res = p; p += pn;
  L.Xp = p; p += pn;
  L.K = p; p += pad32((size_t)S->n * S->maxc);
  L.pv = p; p += pz;
  L.q = p; p += pz;
  L.cn = p; p += pz;
  L.x = p; p += pz;
  L.b = p; p += pz;
  L.r = p; p += pz;
  L.cp = p; p += pz;
  L.Ap = p;
  return L;
}

inline Twin twin_of(const HazanState* S) {
  const CdState& C = S->twin;
  return Twin{C.rptr.as<int64_t>(), C.ridx.as<int32_t>(), C.rval.as<double>(), C.cptr.as<int64_t>(), C.crow.as<int32_t>(), C.cval.as<double>(), S->n, S->d};
}

struct Parts {
  double *p0, *p1, *p2, *p3;
};
inline Parts parts_of(const HazanState* S) {
  double* p = S->part.as<double>();
  return Parts{p, p + S->n_part, p + 2 * S->n_part, p + 3 * S->n_part};
}

#define HZ_LAUNCH(kern, grid, block, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(block), 0, st, __VA_ARGS__)

}  // namespace
}  // namespace nfm
