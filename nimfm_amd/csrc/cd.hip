// nimfm_amd/csrc/cd.hip -- coordinate descent for FactorizationMachines (newCD, optimizer/cd.nim; fitLinearCD /
// fitInterceptCD, optimizer/fit_linear.nim:5-37) as a level schedule over the features.
//
// The reference walks the features j = 0 .. nFeatures-1 one after another; the step of feature j reads and writes the
// per-sample state (yPred[i], cacheDeg2[i] or A[i, 0..deg]) only for the samples i of column j.  Each feature gets a
// level, 1 + the largest level among the earlier features it shares a sample with (0 for an empty column): the features of
// one level share no sample, and every sample sees its features' steps in ascending j, as in the reference's loop.  The
// levels run in ascending order, the features of one level in parallel -- one wavefront per feature, whose lanes gather
// and form the terms while the sums are formed in column order (an in-order chain over the lanes) -- so with
// -ffp-contract=off every step is the reference's, bit for bit.  Levels of at least kWideMin features are a launch of
// their own; a run of narrower levels is walked by one workgroup with a workgroup barrier between levels.  The dummy
// features of fitLower = augment (a column over every sample) and the intercept are one workgroup each, summed with a
// fixed tree: deterministic, but not the reference's rounding.
//
// Proximal coordinate descent (newPCD, optimizer/pcd.nim) is the same iteration with a proximal step
// per feature: plain CD is the regulariser kRegCd of the same kernels.  L1 and row-wise SquaredL12 keep the level
// schedule; column-wise SquaredL12 and OmegaTI read a running value over every earlier feature and run a run schedule.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cd.h"
#include "cd_dev.h"
#include "fm_device.h"

namespace nfm {
using namespace dev;

namespace {

// one (order, component) sweep
struct CdComp {
  double* P;  // P of the component: the parameter of feature j is P[(b * bs + j * rs) * Kp]
  int64_t b, bs, rs;
  int32_t Kp, deg, n_aug, pad_;
  int64_t vbase;  // index in `out` of this sweep's feature 0
  __device__ double& at(int64_t j) const { return P[(size_t)(b * bs + j * rs) * Kp]; }
};

// the parameter P[o][s][j] of the reference layout on the device (ModelView::kc blocks of M.k factors)
__device__ __forceinline__ double p_ref(const ModelView& M, int o, int s, int64_t j) {
  return M.P[M.row((int64_t)o * M.kc + s / M.k, j) * M.Kp + s % M.k];
}

// cd.nim:133-153: yPred = linear(X, w) (per sample, ascending j) + intercept, then + anova(...)[degree - order] for every
// order and component, the dummy features included (kernels.nim:22-43, its degree-2 finalisation too)
__global__ void k_cd_init_yp(CdDev D, ModelView M, int nc, int no) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const int64_t q0 = D.rptr[i], q1 = D.rptr[i + 1];
  double acc = 0.0;
  for (int64_t q = q0; q < q1; ++q) acc += D.rval[q] * M.w[D.ridx[q]];
  acc += M.sc[SC_INTERCEPT];
  for (int o = 0; o < no; ++o) {
    const int deg = M.degree - o;
    for (int s = 0; s < nc; ++s) {
      if (deg == 2) {
        double a1 = 0.0, a2 = 0.0;
        for (int64_t q = q0; q <= q1 + M.n_aug - 1; ++q) {
          const bool dummy = q >= q1;
          const int64_t j = dummy ? D.d + (q - q1) : D.ridx[q];
          const double v = dummy ? 1.0 : D.rval[q];
          const double p = p_ref(M, o, s, j);
          a1 += p * v;
          const double t = p * v;
          a2 += t * t;
        }
        acc += (a1 * a1 - a2) / 2.0;
      } else {
        double A[kCdMaxDeg + 1];
        A[0] = 1.0;
        for (int t = 1; t <= deg; ++t) A[t] = 0.0;
        for (int64_t q = q0; q <= q1 + M.n_aug - 1; ++q) {
          const bool dummy = q >= q1;
          const int64_t j = dummy ? D.d + (q - q1) : D.ridx[q];
          const double v = dummy ? 1.0 : D.rval[q];
          const double p = p_ref(M, o, s, j);
          for (int t = 0; t < deg; ++t) A[deg - t] += A[deg - t - 1] * p * v;
        }
        acc += A[deg];
      }
    }
  }
  D.yp[i] = acc;
}

// colNormSq = norm(X, p = 2, axis = 0)^2 (extmath.nim:151-163, cd.nim:140-142): the square of a square root
__global__ void k_cd_colsq(CdDev D, double* colsq) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= D.d) return;
  double s = 0.0;
  for (int64_t q = D.cptr[j]; q < D.cptr[j + 1]; ++q) s += D.cval[q] * D.cval[q];
  const double r = sqrt(s);
  colsq[j] = r * r;
}

// the cache of one component, per sample in ascending j, dummies last: cacheDeg2 (cd.nim:84-88) or anova's A (kernels.nim:22-43,
// product order (A * P) * val)
__global__ void k_cd_cache(CdDev D, CdComp C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const int64_t q0 = D.rptr[i], q1 = D.rptr[i + 1];
  if (C.deg == 2) {
    double c = 0.0;
    for (int64_t q = q0; q < q1; ++q) c += D.rval[q] * C.at(D.ridx[q]);
    for (int a = 0; a < C.n_aug; ++a) c += 1.0 * C.at(D.d + a);
    D.cache[i] = c;
    return;
  }
  const int deg = C.deg;
  double A[kCdMaxDeg + 1];
  A[0] = 1.0;
  for (int t = 1; t <= deg; ++t) A[t] = 0.0;
  for (int64_t q = q0; q <= q1 + C.n_aug - 1; ++q) {
    const bool dummy = q >= q1;
    const int64_t j = dummy ? D.d + (q - q1) : D.ridx[q];
    const double v = dummy ? 1.0 : D.rval[q];
    const double p = C.at(j);
    for (int t = 0; t < deg; ++t) A[deg - t] += A[deg - t - 1] * p * v;
  }
  double* Ai = D.A + (size_t)i * D.A_ld;
  for (int t = 0; t <= deg; ++t) Ai[t] = A[t];
}

// computeDerivative (cd.nim:24-28): dA[0 .. deg) of sample i, with the OLD psj
__device__ __forceinline__ void cd_derivative(const double* Ai, double psj, double v, int deg, double (&dA)[kCdMaxDeg]) {
  dA[0] = v;
  for (int g = 1; g < deg; ++g) dA[g] = v * (Ai[g] - psj * dA[g - 1]);
}

// lane l's value to the whole wavefront (l a constant after unrolling: v_readlane, no LDS round trip as with __shfl)
__device__ __forceinline__ double lane_d(double v, int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the regulariser of a sweep, as a template parameter: kRegCd is plain CD (no proximal step), the others newPCD's
// (pcd.nim:38-104).  L1 and SquaredL12 row-wise read only the feature's own values (level schedule); SquaredL12
// column-wise and OmegaTI read a running value over every earlier feature (run schedule, pcd chain below).
enum { kRegCd = 0, kRegL1 = 1, kRegSqRow = 2, kRegSqCol = 3, kRegTI = 4 };

// PCD's device state next to CdDev (plain CD's kernels take it last and do not read it)
struct PcdDev {
  double gn;        // gamma * n (pcd.nim:137)
  double* rcache;   // [d + nAug]: SquaredL12 row-wise, cache[j] (squaredl12.nim:166-172,184-188)
  double* su;       // [d + nAug] each, the run schedule's hand-over between its phases: update (before the division),
  double* sinv;     //   invStepSize,
  double* spsj;     //   the old P[s, j],
  double* sdelta;   //   psj - P_new
  double* chain;    // the chained regularisers' running state of the component (ChainState)
  const int64_t* roff;
};

// SquaredL12 column-wise: c[0] = cache[0]; OmegaTI: c = cache[0 .. deg], dc = dcache[0 .. deg] (omegati.nim:40-66)
struct ChainState {
  double c[kCdMaxDeg + 1], dc[kCdMaxDeg + 1];
};

__device__ __forceinline__ void chain_load(ChainState& st, const double* g) {
  for (int t = 0; t <= kCdMaxDeg; ++t) {
    st.c[t] = g[t];
    st.dc[t] = g[kCdMaxDeg + 1 + t];
  }
}

__device__ __forceinline__ void chain_store(const ChainState& st, double* g) {
  for (int t = 0; t <= kCdMaxDeg; ++t) {
    g[t] = st.c[t];
    g[kCdMaxDeg + 1 + t] = st.dc[t];
  }
}

// the proximal step of a local regulariser (pcd.nim:58,101): L1 (l1.nim:25-27) or SquaredL12 row-wise
// (squaredl12.nim:127-131: dcache = cache[j] - absp[j], the product 2 * lam * dcache before the division)
template <int REG>
__device__ __forceinline__ double prox_local(const PcdDev& R, int64_t j, double psj, double u, double lam) {
  if constexpr (REG == kRegL1) {
    return soft_threshold(psj - u, lam);
  } else {
    const double dcache = R.rcache[j] - fabs(psj);
    return soft_threshold((psj - u) / (1 + 2 * lam), 2 * lam * dcache / (1 + 2 * lam));
  }
}

// the proximal step of a chained regulariser with its cache hooks: prox, then updateCacheCD (pcd.nim:58,74,101,107).
// absp[j] is |psj|: computeCacheCD takes it at the component's start, and feature j steps once per component.
template <int REG>
__device__ __forceinline__ double prox_chain(ChainState& st, int deg, double psj, double u, double lam) {
  const double absp = fabs(psj);
  if constexpr (REG == kRegSqCol) {  // squaredl12.nim:127-131,184-188 with i = 0
    const double dcache = st.c[0] - absp;
    const double pn = soft_threshold((psj - u) / (1 + 2 * lam), 2 * lam * dcache / (1 + 2 * lam));
    st.c[0] -= absp;
    st.c[0] += fabs(pn);
    return pn;
  } else {  // omegati.nim:58-66 (prox, dcache clamped at 0), then :53-55 (updateCacheCD)
    for (int g = 2; g <= deg; ++g) {
      st.dc[g] = st.c[g - 1] - st.dc[g - 1] * absp;
      if (st.dc[g] < 0) st.dc[g] = 0.0;
    }
    const double pn = soft_threshold(psj - u, lam * st.dc[deg]);
    const double ap = fabs(pn);
    for (int g = 1; g < deg; ++g) st.c[g] = st.dc[g + 1] + st.dc[g] * ap;
    return pn;
  }
}

// one feature's gradient, one wavefront: update (before the division) and invStepSize.  MODE 1: the linear term
// (fitLinearCD, fit_linear.nim:5-27); 2: degree 2 (epochDeg2, cd.nim:90-107); 3: degree >= 3 (update, cd.nim:31-48).
// The sums run over the column in ascending sample order.
template <int MODE>
__device__ __forceinline__ void cd_grad(const CdDev& D, const CdComp& C, int64_t j, int lane, double& psj_out, double& upd_out,
                                        double& inv_out) {
  const int64_t c0 = D.cptr[j], c1 = D.cptr[j + 1];
  const double psj = MODE == 1 ? D.w[j] : C.at(j);
  double upd = (MODE == 1 ? D.an : D.bn) * psj, inv = 0.0;
  for (int64_t base = c0; base < c1; base += kWave) {
    const int64_t q = base + lane;
    double t1 = 0.0, t2 = 0.0;
    if (q < c1) {
      const int64_t i = D.crow[q];
      const double v = D.cval[q];
      const double dl = dloss_at(D, i);
      if (MODE == 1) {
        t1 = dl * v;
      } else if (MODE == 2) {
        const double dA = (D.cache[i] - psj * v) * v;
        t1 = dl * dA;
        t2 = dA * dA;
      } else {
        double dA[kCdMaxDeg];
        cd_derivative(D.A + (size_t)i * D.A_ld, psj, v, C.deg, dA);
        t1 = dl * dA[C.deg - 1];
        t2 = dA[C.deg - 1] * dA[C.deg - 1];
      }
    }
    const int cnt = (int)(c1 - base < kWave ? c1 - base : kWave);
#pragma unroll
    for (int l = 0; l < kWave; ++l) {  // the reference's order: one term after the other
      if (l < cnt) {
        upd += lane_d(t1, l);
        if (MODE != 1) inv += lane_d(t2, l);
      }
    }
  }
  if (MODE == 1) {
    inv = D.mu * D.colsq[j] + D.an;
  } else {
    inv *= D.mu;
    inv += D.bn;
  }
  psj_out = psj;
  upd_out = upd;
  inv_out = inv;
}

// one feature's synchronisation with the step u (the old psj for the derivative), one wavefront over its column
template <int MODE>
__device__ __forceinline__ void cd_sync(const CdDev& D, const CdComp& C, int64_t j, int lane, double psj, double u) {
  const int64_t c0 = D.cptr[j], c1 = D.cptr[j + 1];
  for (int64_t q = c0 + lane; q < c1; q += kWave) {
    const int64_t i = D.crow[q];
    const double v = D.cval[q];
    if (MODE == 1) {
      D.yp[i] -= u * v;
    } else if (MODE == 2) {
      D.yp[i] -= u * (D.cache[i] - psj * v) * v;
      D.cache[i] -= u * v;
    } else {  // synchronize (cd.nim:67-73): A[i, g] is read for dA[g] before it is decremented
      double* Ai = D.A + (size_t)i * D.A_ld;
      const int deg = C.deg;
      double dA[kCdMaxDeg];
      dA[0] = v;
      for (int g = 1; g < deg; ++g) {
        dA[g] = v * (Ai[g] - psj * dA[g - 1]);
        Ai[g] -= u * dA[g - 1];
      }
      Ai[deg] -= u * dA[deg - 1];
      D.yp[i] -= u * dA[deg - 1];
    }
  }
}

// whether a feature's step is skipped at invStepSize < 1e-12: for CD (kRegCd) in fitLinearCD and epochDeg2 only (MODE 1,
// 2; the general epoch does not skip), for PCD at every MODE (pcd.nim:57,100)
template <int MODE, int REG>
__device__ __forceinline__ bool cd_skip(double inv) {
  return (REG != kRegCd || MODE != 3) && inv < 1e-12;
}

// one feature's step from update (before the division) and invStepSize: P_new and the delta u that viol and the
// synchronisation use.  CD: u = update / invStepSize, P_new = psj - u.  A local regulariser of PCD: P_new by the prox,
// u = psj - P_new (pcd.nim:58-74,101-107).  Each formula is the reference's: psj - (psj - u) is not u in floating point.
template <int REG>
__device__ __forceinline__ void cd_step(const PcdDev& R, int64_t j, double psj, double upd, double inv, double& pn, double& u) {
  if constexpr (REG == kRegCd) {
    u = upd / inv;
    pn = psj - u;
  } else {
    const double lam = R.gn / inv;
    pn = prox_local<REG>(R, j, psj, upd / inv, lam);
    u = psj - pn;
  }
}

// SquaredL12 row-wise, updateCacheCD on cache[j] (squaredl12.nim:184-188): two roundings, as the reference's -= then +=
__device__ __forceinline__ void rcache_update(const PcdDev& R, int64_t j, double psj, double pn) {
  double c = R.rcache[j] - fabs(psj);
  c += fabs(pn);
  R.rcache[j] = c;
}

// one feature's step, one wavefront: the gradient, the skip, the step (CD's, or PCD's with a local regulariser), viol
// and the synchronisation.  MODE 1: the linear term (fitLinearCD, fit_linear.nim:5-27, always CD's step); 2: degree 2
// (epochDeg2, cd.nim:90-107); 3: degree >= 3 (update + synchronize, cd.nim:31-74).  PCD: pcd.nim:55-74,99-107.
template <int MODE, int REG>
__device__ __forceinline__ void cd_feature(const CdDev& D, const CdComp& C, int64_t j, int lane, const PcdDev& R) {
  double psj, upd, inv;
  cd_grad<MODE>(D, C, j, lane, psj, upd, inv);
  if (cd_skip<MODE, REG>(inv)) return;
  double pn, u;
  cd_step<REG>(R, j, psj, upd, inv, pn, u);
  if (lane == 0) {
    if (MODE == 1) {
      D.w[j] = pn;
      D.out[1 + j] = fabs(u);
    } else {
      C.at(j) = pn;
      D.out[C.vbase + j] = fabs(u);
    }
    if constexpr (REG == kRegSqRow) rcache_update(R, j, psj, pn);
  }
  cd_sync<MODE>(D, C, j, lane, psj, u);
}

// one wide level: features order[f0 .. f1), one wavefront each.  R (unused by CD) is the last parameter, so that CD's
// kernel arguments keep their offsets.
template <int MODE, int REG>
__global__ void __launch_bounds__(kBlock) k_cd_level(CdDev D, CdComp C, const int32_t* order, int64_t f0, int64_t f1, PcdDev R) {
  const int64_t f = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (f >= f1) return;
  cd_feature<MODE, REG>(D, C, order[f], threadIdx.x % kWave, R);
}

// a run of narrow levels g0 .. g1-1, walked by ONE workgroup: a barrier between levels
template <int MODE, int REG>
__global__ void __launch_bounds__(kNarrowBlock) k_cd_levels(CdDev D, CdComp C, const int32_t* order, const int64_t* goff, int64_t g0,
                                                            int64_t g1, PcdDev R) {
  const int wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t f1 = goff[g + 1];
    for (int64_t f = goff[g] + wv; f < f1; f += kNarrowWaves) cd_feature<MODE, REG>(D, C, order[f], lane, R);
    __syncthreads();
  }
}

// fitInterceptCD (fit_linear.nim:30-37); the sum over the samples is a fixed tree
__global__ void __launch_bounds__(kNarrowBlock) k_cd_intercept(CdDev D) {
  __shared__ double red[kNarrowBlock];
  double part = 0.0;
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) part += dloss_at(D, i);
  const double S = block_sum(part, red);
  const double b = D.sc[SC_INTERCEPT];
  const double u = (D.a0n * b + S) / (D.mu * (double)D.n + D.a0n);
  if (threadIdx.x == 0) {
    D.sc[SC_INTERCEPT] = b - u;
    D.out[0] = fabs(u);
  }
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) D.yp[i] -= u;
}

// one dummy feature of fitLower = augment (a column of ones over every sample, after all real features): the gradient
// (fixed-tree sums) and the synchronisation, one workgroup
template <int MODE>
__device__ __forceinline__ void dummy_grad(const CdDev& D, const CdComp& C, double psj, double* red, double& upd, double& inv) {
  const double v = 1.0;
  double p1 = 0.0, p2 = 0.0;
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) {
    const double dl = dloss_at(D, i);
    double dd;
    if (MODE == 2) {
      dd = (D.cache[i] - psj * v) * v;
    } else {
      double dA[kCdMaxDeg];
      cd_derivative(D.A + (size_t)i * D.A_ld, psj, v, C.deg, dA);
      dd = dA[C.deg - 1];
    }
    p1 += dl * dd;
    p2 += dd * dd;
  }
  upd = D.bn * psj + block_sum(p1, red);
  inv = block_sum(p2, red);
  inv *= D.mu;
  inv += D.bn;
}

template <int MODE>
__device__ __forceinline__ void dummy_sync(const CdDev& D, const CdComp& C, double psj, double u) {
  const double v = 1.0;
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) {
    if (MODE == 2) {
      D.yp[i] -= u * (D.cache[i] - psj * v) * v;
      D.cache[i] -= u * v;
    } else {
      double* Ai = D.A + (size_t)i * D.A_ld;
      const int deg = C.deg;
      double dA[kCdMaxDeg];
      dA[0] = v;
      for (int g = 1; g < deg; ++g) {
        dA[g] = v * (Ai[g] - psj * dA[g - 1]);
        Ai[g] -= u * dA[g - 1];
      }
      Ai[deg] -= u * dA[deg - 1];
      D.yp[i] -= u * dA[deg - 1];
    }
  }
}

// the dummy feature's step: CD's in every thread; PCD's prox in thread 0 (a chained regulariser continues its running
// state, R.chain), P_new to the workgroup through LDS
template <int MODE, int REG>
__global__ void __launch_bounds__(kNarrowBlock) k_cd_dummy(CdDev D, CdComp C, int64_t j, PcdDev R) {
  __shared__ double red[kNarrowBlock];
  const double psj = C.at(j);
  double upd, inv;
  dummy_grad<MODE>(D, C, psj, red, upd, inv);
  if (cd_skip<MODE, REG>(inv)) return;
  double pn, u;
  if constexpr (REG == kRegCd) {
    cd_step<REG>(R, j, psj, upd, inv, pn, u);
    if (threadIdx.x == 0) {
      C.at(j) = pn;
      D.out[C.vbase + j] = fabs(u);
    }
  } else {
    __shared__ double pn_s;
    if (threadIdx.x == 0) {
      if constexpr (REG == kRegSqCol || REG == kRegTI) {
        ChainState st;
        chain_load(st, R.chain);
        pn = prox_chain<REG>(st, C.deg, psj, upd / inv, R.gn / inv);
        chain_store(st, R.chain);
        u = psj - pn;
      } else {
        cd_step<REG>(R, j, psj, upd, inv, pn, u);
        if constexpr (REG == kRegSqRow) rcache_update(R, j, psj, pn);
      }
      C.at(j) = pn;
      D.out[C.vbase + j] = fabs(u);
      pn_s = pn;
    }
    __syncthreads();
    u = psj - pn_s;
  }
  dummy_sync<MODE>(D, C, psj, u);
}

// ---- PCD only (pcd.nim:38-107): SquaredL12 row-wise's cache and the chained regularisers' run schedule ----
// SquaredL12 row-wise, computeCacheCDAll (squaredl12.nim:166-172): cache[j] = sum_s |P[s, j]|, s ascending, per order
__global__ void k_pcd_rcache(ModelView M, PcdDev R, int o, int nc) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M.da) return;
  double c = 0.0;
  for (int s = 0; s < nc; ++s) c += fabs(p_ref(M, o, s, j));
  R.rcache[j] = c;
}

// computeCacheCD of a chained regulariser (squaredl12.nim:175-181, omegati.nim:36-50): the running state's start over
// every feature in ascending j, one wavefront (the lanes load, the sum runs serially in j order)
template <int REG>
__global__ void __launch_bounds__(kWave) k_pcd_chain_init(CdComp C, PcdDev R, int64_t da) {
  const int lane = threadIdx.x;
  const int deg = C.deg;
  ChainState st;
  for (int t = 0; t <= kCdMaxDeg; ++t) st.c[t] = st.dc[t] = 0.0;
  st.c[0] = REG == kRegTI ? 1.0 : 0.0;
  st.dc[1] = REG == kRegTI ? 1.0 : 0.0;
  for (int64_t base = 0; base < da; base += kWave) {
    const double a = base + lane < da ? fabs(C.at(base + lane)) : 0.0;
    const int cnt = (int)(da - base < kWave ? da - base : kWave);
    for (int l = 0; l < cnt; ++l) {
      const double al = lane_d(a, l);
      if constexpr (REG == kRegSqCol) {
        st.c[0] += al;  // sum(self.absp)
      } else {
        for (int t = 0; t < deg; ++t) st.c[deg - t] += st.c[deg - t - 1] * al;
      }
    }
  }
  if (lane == 0) chain_store(st, R.chain);
}

// the run schedule's phase (a): features f0 .. f1 (one run), one wavefront each: update and invStepSize, no parameter written
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_pcd_grad(CdDev D, CdComp C, PcdDev R, int64_t f0, int64_t f1) {
  const int64_t j = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (j >= f1) return;
  const int lane = threadIdx.x % kWave;
  double psj, upd, inv;
  cd_grad<MODE>(D, C, j, lane, psj, upd, inv);
  if (lane == 0) {
    R.su[j] = upd;
    R.sinv[j] = inv;
    R.spsj[j] = psj;
  }
}

// phase (b): one workgroup; the run's (update, inv, psj) staged in LDS a chunk at a time, then ONE lane walks the
// chain in ascending j (skip, prox, updateCacheCD) and the workgroup writes P_new, |psj - P_new| and the delta
template <int REG>
__global__ void __launch_bounds__(kNarrowBlock) k_pcd_chain(CdDev D, CdComp C, PcdDev R, int64_t f0, int64_t f1) {
  __shared__ double su[kNarrowBlock], si[kNarrowBlock], sp[kNarrowBlock], sn[kNarrowBlock];
  ChainState st;
  if (threadIdx.x == 0) chain_load(st, R.chain);
  for (int64_t base = f0; base < f1; base += kNarrowBlock) {
    const int cnt = (int)(f1 - base < kNarrowBlock ? f1 - base : kNarrowBlock);
    const int t = threadIdx.x;
    if (t < cnt) {
      su[t] = R.su[base + t];
      si[t] = R.sinv[base + t];
      sp[t] = R.spsj[base + t];
    }
    __syncthreads();
    if (t == 0) {
      for (int f = 0; f < cnt; ++f) {
        const double inv = si[f];
        if (inv < 1e-12) continue;  // neither prox nor updateCacheCD (pcd.nim:57,100)
        sn[f] = prox_chain<REG>(st, C.deg, sp[f], su[f] / inv, R.gn / inv);
      }
    }
    __syncthreads();
    if (t < cnt && !(si[t] < 1e-12)) {
      const double psj = sp[t], pn = sn[t];
      C.at(base + t) = pn;
      D.out[C.vbase + base + t] = fabs(psj - pn);
      R.sdelta[base + t] = psj - pn;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) chain_store(st, R.chain);
}

// phase (c): one wavefront per feature synchronises yPred and cacheDeg2 / A with psj - P_new (the old psj for dA)
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_pcd_sync(CdDev D, CdComp C, PcdDev R, int64_t f0, int64_t f1) {
  const int64_t j = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (j >= f1) return;
  if (R.sinv[j] < 1e-12) return;
  cd_sync<MODE>(D, C, j, threadIdx.x % kWave, R.spsj[j], R.sdelta[j]);
}

// a sequence of narrow runs r0 .. r1-1 (each < kWideMin features), walked by ONE workgroup: (a) into LDS, a barrier,
// (b) by thread 0 with the running state in its registers, a barrier, (c), a barrier
template <int MODE, int REG>
__global__ void __launch_bounds__(kNarrowBlock) k_pcd_runs(CdDev D, CdComp C, PcdDev R, int64_t r0, int64_t r1) {
  __shared__ double su[kWideMin], si[kWideMin], sp[kWideMin], sd[kWideMin];
  const int wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  ChainState st;
  if (threadIdx.x == 0) chain_load(st, R.chain);
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t f0 = R.roff[r];
    const int cnt = (int)(R.roff[r + 1] - f0);  // < kWideMin (the host cuts wider runs into launches of their own)
    for (int f = wv; f < cnt; f += kNarrowWaves) {
      double psj, upd, inv;
      cd_grad<MODE>(D, C, f0 + f, lane, psj, upd, inv);
      if (lane == 0) {
        su[f] = upd;
        si[f] = inv;
        sp[f] = psj;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int f = 0; f < cnt; ++f) {
        const double inv = si[f];
        if (inv < 1e-12) continue;
        const double psj = sp[f];
        const double pn = prox_chain<REG>(st, C.deg, psj, su[f] / inv, R.gn / inv);
        C.at(f0 + f) = pn;
        D.out[C.vbase + f0 + f] = fabs(psj - pn);
        sd[f] = psj - pn;
      }
    }
    __syncthreads();
    for (int f = wv; f < cnt; f += kNarrowWaves)
      if (!(si[f] < 1e-12)) cd_sync<MODE>(D, C, f0 + f, lane, sp[f], sd[f]);
    __syncthreads();
  }
  if (threadIdx.x == 0) chain_store(st, R.chain);
}

// sum_i loss(y_i, yPred_i) after the iteration (cd.nim:177-181), a fixed tree
__global__ void __launch_bounds__(kNarrowBlock) k_cd_loss(CdDev D, double* dst) {
  __shared__ double red[kNarrowBlock];
  double part = 0.0;
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) part += loss_value(D.loss, D.lp, target_of(D.y[i], D.task), D.yp[i]);
  const double S = block_sum(part, red);
  if (threadIdx.x == 0) *dst = S;
}

double loss_mu(int loss) {  // loss.nim: mu
  switch (loss) {
    case NFM_LOSS_SQUARED_HINGE: return 2.0;
    case NFM_LOSS_LOGISTIC: return 0.25;
    default: return 1.0;
  }
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

CdDev dev_view(const CsrView& X, const ModelView& M, const CdParams& P, CdState* S) {
  CdDev D{};
  D.rptr = S->rptr.as<int64_t>(); D.ridx = S->ridx.as<int32_t>(); D.rval = S->rval.as<double>();
  D.cptr = S->cptr.as<int64_t>(); D.crow = S->crow.as<int32_t>(); D.cval = S->cval.as<double>();
  D.y = X.y; D.yp = S->yp.as<double>(); D.cache = S->cache.as<double>(); D.A = S->A.as<double>();
  D.colsq = S->colsq.as<double>(); D.out = S->out.as<double>(); D.w = M.w; D.sc = M.sc;
  D.n = X.n; D.d = X.d; D.task = M.task; D.loss = P.loss; D.A_ld = M.degree + 1;
  D.lp = P.loss_param; D.mu = S->mu; D.a0n = S->a0n; D.an = S->an; D.bn = S->bn;
  return D;
}

// the level sweeps over the real features of one (order, component), or of the linear term
template <int MODE, int REG>
int sweep_levels(nfm_ctx* ctx, const CdDev& D, const CdComp& C, const PcdDev& R, CdState* S) {
  hipStream_t st = ctx->stream;
  const int64_t G = (int64_t)S->goff_h.size() - 1;
  const int32_t* order = S->order.as<int32_t>();
  for (int64_t g = 0; g < G;) {
    const int64_t width = S->goff_h[g + 1] - S->goff_h[g];
    if (width >= kWideMin) {
      hipLaunchKernelGGL((k_cd_level<MODE, REG>), dim3(blocks_for(width, kWavesPerBlock)), dim3(kBlock), 0, st, D, C, order, S->goff_h[g],
                         S->goff_h[g + 1], R);
      ++g;
    } else {
      int64_t g1 = g;
      while (g1 < G && S->goff_h[g1 + 1] - S->goff_h[g1] < kWideMin) ++g1;
      hipLaunchKernelGGL((k_cd_levels<MODE, REG>), dim3(1), dim3(kNarrowBlock), 0, st, D, C, order, S->goff.as<int64_t>(), g, g1, R);
      g = g1;
    }
  }
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

PcdDev pcd_view(CdState* S) {
  PcdDev R{};
  R.gn = S->gn;
  R.rcache = S->rcache.as<double>();
  const int64_t da = std::max<int64_t>(S->sgrad.bytes / (4 * sizeof(double)), 1);
  double* g = S->sgrad.as<double>();
  R.su = g;
  R.sinv = g + da;
  R.spsj = g + 2 * da;
  R.sdelta = g + 3 * da;
  R.chain = S->chain.as<double>();
  R.roff = S->roff.as<int64_t>();
  return R;
}

// PCD with a chained regulariser: the run schedule.  A wide run is three launches (gradients, chain, synchronisation);
// consecutive narrow runs are one workgroup's walk
template <int MODE, int REG>
int sweep_runs(nfm_ctx* ctx, const CdDev& D, const CdComp& C, const PcdDev& R, CdState* S) {
  hipStream_t st = ctx->stream;
  const int64_t NR = (int64_t)S->roff_h.size() - 1;
  for (int64_t r = 0; r < NR;) {
    const int64_t f0 = S->roff_h[r], f1 = S->roff_h[r + 1], width = f1 - f0;
    if (width >= kWideMin) {
      const dim3 grid(blocks_for(width, kWavesPerBlock));
      hipLaunchKernelGGL(k_pcd_grad<MODE>, grid, dim3(kBlock), 0, st, D, C, R, f0, f1);
      hipLaunchKernelGGL(k_pcd_chain<REG>, dim3(1), dim3(kNarrowBlock), 0, st, D, C, R, f0, f1);
      hipLaunchKernelGGL(k_pcd_sync<MODE>, grid, dim3(kBlock), 0, st, D, C, R, f0, f1);
      ++r;
    } else {
      int64_t r1 = r;
      while (r1 < NR && S->roff_h[r1 + 1] - S->roff_h[r1] < kWideMin) ++r1;
      hipLaunchKernelGGL((k_pcd_runs<MODE, REG>), dim3(1), dim3(kNarrowBlock), 0, st, D, C, R, r, r1);
      r = r1;
    }
  }
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// one (order, component) P sweep with regulariser REG (kRegCd: plain CD): the real features -- the level schedule, or a
// chained regulariser's start and the run schedule -- then the dummy features
template <int MODE, int REG>
int sweep(nfm_ctx* ctx, const CsrView& X, const CdDev& D, const CdComp& C, const PcdDev& R, CdState* S) {
  hipStream_t st = ctx->stream;
  if constexpr (REG == kRegSqCol || REG == kRegTI) {
    hipLaunchKernelGGL(k_pcd_chain_init<REG>, dim3(1), dim3(kWave), 0, st, C, R, X.d + C.n_aug);
    NFM_TRY((sweep_runs<MODE, REG>(ctx, D, C, R, S)));
  } else {
    NFM_TRY((sweep_levels<MODE, REG>(ctx, D, C, R, S)));
  }
  for (int a = 0; a < C.n_aug; ++a) hipLaunchKernelGGL((k_cd_dummy<MODE, REG>), dim3(1), dim3(kNarrowBlock), 0, st, D, C, X.d + a, R);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

template <int MODE>
int sweep_reg(nfm_ctx* ctx, const CsrView& X, const CdDev& D, const CdComp& C, const PcdDev& R, const CdParams& P, CdState* S) {
  switch (P.reg) {
    case kCdNoReg: return sweep<MODE, kRegCd>(ctx, X, D, C, R, S);
    case NFM_REG_L1: return sweep<MODE, kRegL1>(ctx, X, D, C, R, S);
    case NFM_REG_SQUAREDL12:
      return P.reg_transpose ? sweep<MODE, kRegSqCol>(ctx, X, D, C, R, S) : sweep<MODE, kRegSqRow>(ctx, X, D, C, R, S);
    case NFM_REG_OMEGATI: return sweep<MODE, kRegTI>(ctx, X, D, C, R, S);
    default: NFM_CHECK(false, NFM_ERR_UNSUPPORTED, "regularizer %d has no PCD step", P.reg);
  }
  return NFM_OK;
}

CdComp comp_view(const ModelView& M, int o, int s, int nc) {
  CdComp C{};
  C.b = (int64_t)o * M.kc + s / M.k;
  C.P = M.P + s % M.k;
  C.bs = M.bs; C.rs = M.rs; C.Kp = M.Kp;
  C.deg = M.degree - o;
  C.n_aug = M.n_aug;
  C.vbase = 1 + M.d + ((int64_t)o * nc + s) * M.da;
  return C;
}

// every launch of one iteration, in the reference's order (cd.nim:156-175)
int issue_iteration(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int nc, const CdParams& P, CdState* S) {
  hipStream_t st = ctx->stream;
  CdDev D = dev_view(X, M, P, S);
  NFM_HIP_CHECK(hipMemsetAsync(S->out.p, 0, sizeof(double) * S->n_out, st));
  if (M.fit_intercept) hipLaunchKernelGGL(k_cd_intercept, dim3(1), dim3(kNarrowBlock), 0, st, D);
  const PcdDev R = P.reg != kCdNoReg && !P.block ? pcd_view(S) : PcdDev{};
  if (M.fit_linear) NFM_TRY((sweep_levels<1, kRegCd>(ctx, D, CdComp{}, R, S)));
  // newPBCD (pbcd.nim:292-299): the intercept and the w sweep above are CD's, the P sweeps step whole rows (pbcd.hip)
  const int no = P.block ? 0 : M.nb / M.kc;
  if (P.block) NFM_TRY(pbcd_issue_orders(ctx, X, M, nc, P, S, D));
  for (int o = 0; o < no; ++o) {
    // computeCacheCDAll (pcd.nim:48,84): SquaredL12 row-wise sums |P| over the order's components
    if (P.reg == NFM_REG_SQUAREDL12 && !P.reg_transpose)
      hipLaunchKernelGGL(k_pcd_rcache, dim3(blocks_for(M.da, kBlock)), dim3(kBlock), 0, st, M, R, o, nc);
    for (int s = 0; s < nc; ++s) {
      const CdComp C = comp_view(M, o, s, nc);
      hipLaunchKernelGGL(k_cd_cache, dim3(blocks_for(X.n, kBlock)), dim3(kBlock), 0, st, D, C);
      NFM_TRY(C.deg == 2 ? sweep_reg<2>(ctx, X, D, C, R, P, S) : sweep_reg<3>(ctx, X, D, C, R, P, S));
    }
  }
  hipLaunchKernelGGL(k_cd_loss, dim3(1), dim3(kNarrowBlock), 0, st, D, S->out.as<double>() + S->n_out - 1);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

template <class T>
int upload(nfm_ctx* ctx, DevBuf& b, const std::vector<T>& h) {
  NFM_TRY(b.alloc(sizeof(T) * std::max<size_t>(h.size(), 1)));
  if (!h.empty()) NFM_HIP_CHECK(hipMemcpyAsync(b.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->stream));
  return NFM_OK;
}

}  // namespace

// fitInterceptCD and fitLinearCD (fit_linear.nim:5-37) for a solver that keeps yPred itself: D.yp, D.colsq and D.out [1 + d] are
// the caller's, S holds the twin and the levels
int cd_issue_intercept(nfm_ctx* ctx, const CdDev& D) {
  hipLaunchKernelGGL(k_cd_intercept, dim3(1), dim3(kNarrowBlock), 0, ctx->stream, D);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

int cd_issue_linear(nfm_ctx* ctx, const CdDev& D, CdState* S) { return sweep_levels<1, kRegCd>(ctx, D, CdComp{}, PcdDev{}, S); }

double cd_loss_mu(int loss) { return loss_mu(loss); }

void CdState::drop_graph() {
  if (graph_exec) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(graph_exec));
  graph_exec = nullptr;
  graph_uid = 0;
}

CdState::~CdState() {
  drop_graph();
  if (out_h) (void)hipHostFree(out_h);
}

// The schedule: the rows with ascending column ids, the column twin (sample ids ascending), the feature levels and the
// features sorted by (level, j).  O(nnz) on the host, once per dataset: the arrays come back from the device for it.
int cd_schedule(nfm_ctx* ctx, const CsrView& X, uint64_t uid, int n_aug, CdState* S, int64_t* n_levels, int64_t* widest, bool runs) {
  if (!(S->sched_ready && S->sched_uid == uid)) {
    S->sched_ready = false;
    S->drop_graph();
    S->fit_ready = false;
    const int64_t n = X.n, d = X.d, nnz = X.nnz;
    hipStream_t st = ctx->stream;
    std::vector<int64_t> rp((size_t)n + 1);
    std::vector<int32_t> ri((size_t)nnz);
    std::vector<double> rv((size_t)nnz);
    NFM_HIP_CHECK(hipMemcpyAsync(rp.data(), X.indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, st));
    if (nnz > 0) {
      NFM_HIP_CHECK(hipMemcpyAsync(ri.data(), X.indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, st));
      NFM_HIP_CHECK(hipMemcpyAsync(rv.data(), X.data, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
    }
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    NFM_CHECK(rp[0] == 0 && rp[n] == nnz, NFM_ERR_INVALID, "bad indptr");
    // rows not sorted by column id get a sorted copy: the per-sample sums follow ascending j
    std::vector<std::pair<int32_t, double>> tmp;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t q0 = rp[i], q1 = rp[i + 1];
      NFM_CHECK(q0 <= q1 && q1 <= nnz, NFM_ERR_INVALID, "bad indptr at row %lld", (long long)i);
      bool sorted = true;
      for (int64_t q = q0; q < q1; ++q) {
        NFM_CHECK(ri[q] >= 0 && ri[q] < d, NFM_ERR_INVALID, "column id %d out of range in row %lld", ri[q], (long long)i);
        if (q > q0 && ri[q] <= ri[q - 1]) sorted = false;
      }
      if (sorted) continue;
      tmp.clear();
      for (int64_t q = q0; q < q1; ++q) tmp.emplace_back(ri[q], rv[q]);
      std::stable_sort(tmp.begin(), tmp.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
      for (size_t t = 0; t < tmp.size(); ++t) {
        NFM_CHECK(t == 0 || tmp[t].first != tmp[t - 1].first, NFM_ERR_UNSUPPORTED, "column id %d repeated in row %lld", tmp[t].first,
                  (long long)i);
        ri[q0 + t] = tmp[t].first;
        rv[q0 + t] = tmp[t].second;
      }
    }
    // the column twin: a counting sort over the rows in ascending i keeps the sample ids ascending inside a column
    std::vector<int64_t> cp((size_t)d + 1, 0);
    for (int64_t q = 0; q < nnz; ++q) ++cp[(size_t)ri[q] + 1];
    for (int64_t j = 0; j < d; ++j) cp[j + 1] += cp[j];
    std::vector<int64_t> nxt(cp.begin(), cp.end() - 1);
    std::vector<int32_t> cr((size_t)nnz);
    std::vector<double> cv((size_t)nnz);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t q = rp[i]; q < rp[i + 1]; ++q) {
        const int64_t pos = nxt[ri[q]]++;
        cr[pos] = (int32_t)i;
        cv[pos] = rv[q];
      }
    // levels: level(j) = 1 + max(last[i] for i in col j), 0 for an empty column; then last[i] = level(j)
    std::vector<int32_t> last((size_t)n, 0), lvl((size_t)d, 0);
    int32_t max_lvl = 0;
    for (int64_t j = 0; j < d; ++j) {
      if (cp[j + 1] == cp[j]) continue;
      int32_t mx = 0;
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) mx = std::max(mx, last[cr[q]]);
      lvl[j] = mx + 1;
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) last[cr[q]] = mx + 1;
      max_lvl = std::max(max_lvl, mx + 1);
    }
    std::vector<int64_t> cnt((size_t)max_lvl + 2, 0);
    for (int64_t j = 0; j < d; ++j) ++cnt[(size_t)lvl[j] + 1];
    for (int32_t l = 0; l <= max_lvl; ++l) cnt[l + 1] += cnt[l];
    std::vector<int32_t> ord((size_t)d);
    {
      std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
      for (int64_t j = 0; j < d; ++j) ord[at[lvl[j]]++] = (int32_t)j;
    }
    // runs (the chained regularisers of PCD): walk j ascending, cut a new run when column j shares a sample with a
    // column of the current run; empty columns join the current run
    S->roff_h.assign(1, 0);
    S->widest_run = 0;
    {
      std::vector<int64_t> mark((size_t)n, -1);
      int64_t run = 0;
      for (int64_t j = 0; j < d; ++j) {
        bool clash = false;
        for (int64_t q = cp[j]; q < cp[j + 1] && !clash; ++q) clash = mark[cr[q]] == run;
        if (clash) {
          S->roff_h.push_back(j);
          ++run;
        }
        for (int64_t q = cp[j]; q < cp[j + 1]; ++q) mark[cr[q]] = run;
      }
      if (d > 0) S->roff_h.push_back(d);
      for (size_t r = 0; r + 1 < S->roff_h.size(); ++r) S->widest_run = std::max(S->widest_run, S->roff_h[r + 1] - S->roff_h[r]);
    }
    S->goff_h.assign(1, 0);
    S->widest = 0;
    for (int32_t l = 0; l <= max_lvl; ++l)
      if (cnt[l + 1] > cnt[l]) {
        S->goff_h.push_back(cnt[l + 1]);
        S->widest = std::max(S->widest, cnt[l + 1] - cnt[l]);
      }
    NFM_TRY(upload(ctx, S->rptr, rp));
    NFM_TRY(upload(ctx, S->ridx, ri));
    NFM_TRY(upload(ctx, S->rval, rv));
    NFM_TRY(upload(ctx, S->cptr, cp));
    NFM_TRY(upload(ctx, S->crow, cr));
    NFM_TRY(upload(ctx, S->cval, cv));
    NFM_TRY(upload(ctx, S->order, ord));
    NFM_TRY(upload(ctx, S->goff, S->goff_h));
    NFM_TRY(upload(ctx, S->roff, S->roff_h));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    S->n = n;
    S->d = d;
    S->nnz = nnz;
    S->sched_uid = uid;
    S->sched_ready = true;
  }
  // the dummy features of fitLower = augment are one level (run) each, after all real features
  if (runs) {
    if (n_levels) *n_levels = (int64_t)S->roff_h.size() - 1 + n_aug;
    if (widest) *widest = std::max<int64_t>(S->widest_run, n_aug > 0 ? 1 : 0);
    return NFM_OK;
  }
  if (n_levels) *n_levels = (int64_t)S->goff_h.size() - 1 + n_aug;
  if (widest) *widest = std::max<int64_t>(S->widest, n_aug > 0 ? 1 : 0);
  return NFM_OK;
}

int cd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, int n_components, const CdParams& P,
                 CdState* S) {
  NFM_CHECK(X.n >= 1, NFM_ERR_INVALID, "nSamples < 1");
  NFM_TRY(cd_schedule(ctx, X, uid, M.n_aug, S, nullptr, nullptr));
  if (S->fit_uid != uid || S->fit_serial != serial) S->drop_graph();  // a captured iteration holds the dataset's pointers
  S->fit_ready = false;
  const double nd = (double)X.n;
  S->a0n = P.alpha0 * nd;
  S->an = P.alpha * nd;
  S->bn = P.beta * nd;
  S->mu = loss_mu(P.loss);
  const int no = M.nb / M.kc;
  S->n_out = 1 + M.d + (int64_t)no * n_components * M.da + 1;
  NFM_TRY(S->yp.ensure(sizeof(double) * X.n));
  NFM_TRY(S->cache.ensure(sizeof(double) * X.n));
  NFM_TRY(S->A.ensure(M.degree >= 3 ? sizeof(double) * X.n * (M.degree + 1) : sizeof(double)));
  NFM_TRY(S->colsq.ensure(sizeof(double) * std::max<int64_t>(M.d, 1)));
  S->gn = P.gamma * nd;
  if (P.reg != kCdNoReg && !P.block) {
    NFM_TRY(S->rcache.ensure(sizeof(double) * std::max<int64_t>(M.da, 1)));
    NFM_TRY(S->chain.ensure(sizeof(double) * 2 * (kCdMaxDeg + 1)));
    if (!S->sgrad.p || S->sgrad.bytes != sizeof(double) * 4 * std::max<int64_t>(M.da, 1)) {  // pcd_view cuts it in four
      S->drop_graph();
      NFM_TRY(S->sgrad.alloc(sizeof(double) * 4 * std::max<int64_t>(M.da, 1)));
    }
  }
  const size_t out_bytes = sizeof(double) * S->n_out;
  if (!S->out.p || S->out.bytes < out_bytes) {
    S->drop_graph();
    NFM_TRY(S->out.alloc(out_bytes));
    if (S->out_h) (void)hipHostFree(S->out_h);
    S->out_h = nullptr;
    NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&S->out_h), out_bytes, hipHostMallocDefault));
  }
  hipStream_t st = ctx->stream;
  const CdDev D = dev_view(X, M, P, S);
  if (M.fit_linear) hipLaunchKernelGGL(k_cd_colsq, dim3(blocks_for(M.d, kBlock)), dim3(kBlock), 0, st, D, S->colsq.as<double>());
  if (P.block)
    NFM_TRY(pbcd_begin_fit(ctx, X, M, n_components, P, S, D));
  else
    hipLaunchKernelGGL(k_cd_init_yp, dim3(blocks_for(X.n, kBlock)), dim3(kBlock), 0, st, D, M, n_components, no);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  S->fit_uid = uid;
  S->fit_serial = serial;
  S->fit_ready = true;
  return NFM_OK;
}

int cd_epoch(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int n_components, const CdParams& P, CdState* S, double* loss_sum,
             double* viol_sum) {
  hipStream_t st = ctx->stream;
  // the whole iteration is one captured graph per (optimizer, dataset); NFM_CD_GRAPH=0 issues the launches one by one
  static const bool use_graph = !(getenv("NFM_CD_GRAPH") && atoi(getenv("NFM_CD_GRAPH")) == 0);
  if (use_graph && !S->graph_exec) {
    NFM_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = issue_iteration(ctx, X, M, n_components, P, S);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc != NFM_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    NFM_HIP_CHECK(e);
    hipGraphExec_t exec = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    NFM_HIP_CHECK(e2);
    S->graph_exec = exec;
    S->graph_uid = S->fit_uid;
    S->graph_serial = S->fit_serial;
  }
  if (use_graph)
    NFM_HIP_CHECK(hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(S->graph_exec), st));
  else
    NFM_TRY(issue_iteration(ctx, X, M, n_components, P, S));
  NFM_HIP_CHECK(hipMemcpyAsync(S->out_h, S->out.p, sizeof(double) * S->n_out, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  // viol in the reference's order (cd.nim:157-171): the intercept's, then fitLinearCD's sum, then one sum per order
  const double* h = S->out_h;
  double viol = 0.0;
  viol += h[0];
  double sw = 0.0;
  for (int64_t j = 0; j < M.d; ++j) sw += h[1 + j];
  viol += sw;
  const int no = M.nb / M.kc;
  for (int o = 0; o < no; ++o) {
    double so = 0.0;
    const double* vo = h + 1 + M.d + (int64_t)o * n_components * M.da;
    for (int64_t t = 0; t < (int64_t)n_components * M.da; ++t) so += vo[t];
    viol += so;
  }
  if (loss_sum) *loss_sum = h[S->n_out - 1];
  if (viol_sum) *viol_sum = viol;
  return NFM_OK;
}

}  // namespace nfm
