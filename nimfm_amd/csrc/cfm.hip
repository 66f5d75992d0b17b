// nimfm_amd/csrc/cfm.hip -- the convex factorization machine (model/convex_factorization_machine.nim) and Hazan's algorithm
// (optimizer/hazan.nim:59-225, tensor/tensor.nim:912-934 powerMethod, :970-1009 cg) for gfx950.
//
// Everything is fp64 and bound by memory.  Two kinds of pass walk the matrix:
//   a row pass: kG lanes take one row, load kG entries at a time (coalesced) and add the products up in storage order --
//     the value every lane of the group ends with is the reference's sequential sum (extmath.nim:93-101, kernels.nim:22-43);
//   a column pass over the column twin, the same way per column (extmath.nim:115-123).
// Sums over n or d are fixed trees: per workgroup a tree over its rows / columns / elements, then one workgroup of
// kNarrowBlock threads sums the workgroups' partials (each thread a strided run, in order) and ends with cd_dev.h's block_sum.
// Nothing is atomic; two runs give the same bits.
// The power method and CG run in chunks of kHazanChunk iterations, each chunk one captured single-stream graph.  Every kernel
// of a chunk reads a stop flag in device memory first and does nothing once it is set; the one-workgroup kernels that own the
// scalars are the only writers of the flags, and every flag is read only by later launches.
#include <math.h>

#include <algorithm>
#include <vector>

#include "cfm_dev.h"

namespace nfm {
namespace {

enum {
  HZ_MAXIT_P = 0, HZ_TOL_P, HZ_P_IT, HZ_P_EVAL, HZ_P_EVAL_OLD, HZ_P_NRM, HZ_P_STOP, HZ_P_DONORM,
  HZ_S, HZ_REPLACED, HZ_STEP, HZ_SCALE, HZ_RESCALE, HZ_TRACE,
  HZ_CG_TOL, HZ_CG_IT, HZ_CG_STOP, HZ_CG_ALPHA, HZ_CG_BETA, HZ_CG_DOTR, HZ_CG_DOUPD, HZ_CG_DOP,
  HZ_LOSS, HZ_COUNT = 32
};

// ---- row pass ----
// out[i] = sum_q rval[q] * v(ridx[q]) (+ 1.0 * extra) (* scale[i]), v(j) = vec[j] / div[j] when div (the right
// preconditioner applied on the fly: the same quotient cg's pPre holds); part0: the workgroups' sums of out (the dummy
// column of ones of hazan.nim:180)
__global__ void __launch_bounds__(kBlock) k_rows(Twin T, const double* vec, const double* div, const double* extra, const double* extra_div,
                                                 const double* scale, double* out, double* part0, const double* flag) {
  __shared__ double red[kGroups];
  if (flag && *flag != 0.0) return;
  const int g = threadIdx.x / kG, gl = threadIdx.x % kG, base = (threadIdx.x % kWave) - gl;
  const int64_t i = (int64_t)blockIdx.x * kGroups + g;
  double v = 0.0;
  if (i < T.n) {
    const int64_t q0 = T.rptr[i], q1 = T.rptr[i + 1];
    if (div)
      v = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { const int32_t j = T.ridx[q]; return T.rval[q] * (vec[j] / div[j]); });
    else
      v = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return T.rval[q] * vec[T.ridx[q]]; });
    if (extra) v += 1.0 * (extra_div ? *extra / *extra_div : *extra);
    if (scale) v *= scale[i];
    if (gl == 0) out[i] = v;
  }
  if (part0) {
    if (gl == 0) red[g] = v;
    const double s = tree(red, kGroups);
    if (threadIdx.x == 0) part0[blockIdx.x] = s;
  }
}

// ---- column pass ----
enum { COL_POWER = 0, COL_CG = 1, COL_B = 2, COL_SQ = 3 };
// out[j] = sum_q cval[q] * src[crow[q]], then
//   COL_POWER: with ignore_diag, minus val * val * res[i] * p[j] entry after entry (hazan.nim:118-121); part0 <- p[j] * out[j],
//              part1 <- out[j]^2
//   COL_CG:    out[j] /= cn[j] (the left preconditioner); part0 <- dv[j] * out[j]
//   COL_B:     part0 <- |out[j]|
//   COL_SQ:    out[j] = sqrt(sum val^2)^2 (norm(X, 2, axis = 0) squared, hazan.nim:93-94)
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_cols(Twin T, const double* src, const double* dv, const double* res, const double* cn, int ignore_diag,
                                                 double* out, double* part0, double* part1, const double* flag) {
  __shared__ double red[kGroups], red2[kGroups];
  if (flag && *flag != 0.0) return;
  const int g = threadIdx.x / kG, gl = threadIdx.x % kG, base = (threadIdx.x % kWave) - gl;
  const int64_t j = (int64_t)blockIdx.x * kGroups + g;
  double a = 0.0, b = 0.0;
  if (j < T.d) {
    const int64_t q0 = T.cptr[j], q1 = T.cptr[j + 1];
    double v;
    if (MODE == COL_SQ) {
      v = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return T.cval[q] * T.cval[q]; });
      v = sqrt(v);
      v *= v;
    } else {
      v = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return T.cval[q] * src[T.crow[q]]; });
    }
    if (MODE == COL_POWER) {
      const double pj = dv[j];
      if (ignore_diag) v = ordered_acc(v, q0, q1, gl, base, [&](int64_t q) { return -(T.cval[q] * T.cval[q] * res[T.crow[q]] * pj); });
      a = pj * v;
      b = v * v;
    } else if (MODE == COL_CG) {
      v /= cn[j];
      a = dv[j] * v;
    } else if (MODE == COL_B) {
      a = fabs(v);
    }
    if (gl == 0) out[j] = v;
  }
  if (MODE != COL_SQ) {
    if (gl == 0) {
      red[g] = a;
      red2[g] = b;
    }
    const double s = tree(red, kGroups);
    if (threadIdx.x == 0) part0[blockIdx.x] = s;
    if (MODE == COL_POWER) {
      const double s2 = tree(red2, kGroups);
      if (threadIdx.x == 0) part1[blockIdx.x] = s2;
    }
  }
}

// ---- power method (tensor.nim:924-933) ----
__global__ void __launch_bounds__(kNarrowBlock) k_power_fin(const double* part0, const double* part1, int64_t np, double* sc) {
  __shared__ double red[kNarrowBlock];
  const bool stopped = sc[HZ_P_STOP] != 0.0;
  __syncthreads();
  if (stopped) {
    if (threadIdx.x == 0) sc[HZ_P_DONORM] = 0.0;
    return;
  }
  const double pq = fin_sum(part0, np, red), qq = fin_sum(part1, np, red);
  if (threadIdx.x == 0) {
    const double it = sc[HZ_P_IT], eval = pq;
    const bool stop = (it > 0.0 && fabs(eval - sc[HZ_P_EVAL_OLD]) < sc[HZ_TOL_P]) || it + 1.0 >= sc[HZ_MAXIT_P];
    sc[HZ_P_EVAL] = eval;
    sc[HZ_P_EVAL_OLD] = eval;
    sc[HZ_P_NRM] = sqrt(qq);
    sc[HZ_P_IT] = it + 1.0;
    sc[HZ_P_STOP] = stop ? 1.0 : 0.0;
    sc[HZ_P_DONORM] = 1.0;
  }
}

__global__ void __launch_bounds__(kBlock) k_power_norm(const double* q, double* p, int64_t d, const double* sc) {
  if (sc[HZ_P_DONORM] == 0.0) return;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < d) p[j] = q[j] / sc[HZ_P_NRM];
}

// ---- the outer iteration's own steps (hazan.nim:144-174) ----
// append (s = n_components, lams[s] = 0) or replace slot argmin(lams) (utils.nim:21-24: the first minimum)
__global__ void k_select(double* lams, int nc, int maxc, double* sc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int s = nc;
  double replaced = 0.0;
  if (nc == maxc) {
    s = 0;
    for (int t = 1; t < nc; ++t)
      if (lams[t] < lams[s]) s = t;
    replaced = 1.0;
  } else {
    lams[s] = 0.0;
  }
  sc[HZ_S] = (double)s;
  sc[HZ_REPLACED] = replaced;
}

// P[s] = p, s = *slot (a device scalar: Hazan's HZ_S, GreedyCD's slot)
__global__ void __launch_bounds__(kBlock) k_set_row(double* P, const double* p, int64_t d, const double* slot) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < d) P[(int64_t)*slot * d + j] = p[j];
}

// K[s] of one component (kernels.nim:22-43 anova, :67-79 poly, degree 2) and what hangs on it.
// init (begin_fit, s = s_fixed): yPredQuad += lams[s] * K[s] (hazan.nim:104-110).
// else (s from sc): yPredQuad loses the replaced slot's old term, gains lams[s] * K[s]; residual = y - yPredQuad - yPredLinear;
// part0 / part1: <d, residual> and ||d||^2 for d = eta * K[s] - yPredQuad (hazan.nim:149,156-162,52-53)
__global__ void __launch_bounds__(kBlock) k_kernel(Twin T, const double* P, const double* lams, int s_fixed, int ignore_diag, double eta,
                                                   const double* yt, const double* ypl, double* ypq, double* res, double* K, double* part0,
                                                   double* part1, const double* sc) {
  __shared__ double red[kGroups], red2[kGroups];
  const bool init = s_fixed >= 0;
  const int s = init ? s_fixed : (int)sc[HZ_S];
  const bool replaced = !init && sc[HZ_REPLACED] != 0.0;
  const int g = threadIdx.x / kG, gl = threadIdx.x % kG, base = (threadIdx.x % kWave) - gl;
  const int64_t i = (int64_t)blockIdx.x * kGroups + g;
  const double* Ps = P + (int64_t)s * T.d;
  double a = 0.0, b = 0.0;
  if (i < T.n) {
    const int64_t q0 = T.rptr[i], q1 = T.rptr[i + 1];
    const double k = kernel_value(T.ridx, T.rval, Ps, q0, q1, gl, base, ignore_diag);
    if (gl == 0) {
      double* Ks = K + (int64_t)s * T.n;
      const double lam = lams[s];
      double v = ypq[i];
      if (replaced) v -= lam * Ks[i];
      Ks[i] = k;
      v += lam * k;
      ypq[i] = v;
      if (!init) {
        const double r = yt[i] - v - ypl[i];
        res[i] = r;
        const double dd = eta * k - v;
        a = dd * r;
        b = dd * dd;
      }
    }
  }
  if (!init) {
    if (gl == 0) {
      red[g] = a;
      red2[g] = b;
    }
    const double s0 = tree(red, kGroups);
    const double s1 = tree(red2, kGroups);
    if (threadIdx.x == 0) {
      part0[blockIdx.x] = s0;
      part1[blockIdx.x] = s1;
    }
  }
}

// computeStepSize (hazan.nim:49-56; Nim's max / min on a NaN quotient give 1.0), the lams update and the rescale (:166-174)
__global__ void __launch_bounds__(kNarrowBlock) k_step(const double* part0, const double* part1, int64_t np, double* lams, int nc, double eta,
                                                       int optimal, double it, double* sc) {
  __shared__ double red[kNarrowBlock];
  const double dot = fin_sum(part0, np, red), dd = fin_sum(part1, np, red);
  if (threadIdx.x != 0) return;
  double step;
  if (optimal) {
    const double nrm = sqrt(dd);
    const double raw = dot / (nrm * nrm);
    const double m = raw <= 1e-10 ? 1e-10 : raw;  // max(1e-10, raw): `if y <= x: x else: y`
    step = m <= 1.0 ? m : 1.0;                    // min(m, 1.0): `if x <= y: x else: y`
  } else {
    step = 2.0 / (it + 2.0);
  }
  const int s = (int)sc[HZ_S];
  for (int t = 0; t < nc; ++t) lams[t] *= (1 - step);
  lams[s] += eta * step;
  double sum = 0.0;
  for (int t = 0; t < nc; ++t) sum += lams[t];
  double f = 1.0, rescale = 0.0;
  if (sum > eta) {
    f = eta / sum;
    rescale = 1.0;
    for (int t = 0; t < nc; ++t) lams[t] *= f;
  }
  double trace = 0.0;
  for (int t = 0; t < nc; ++t) trace += fabs(lams[t]);
  sc[HZ_STEP] = step;
  sc[HZ_SCALE] = f;
  sc[HZ_RESCALE] = rescale;
  sc[HZ_TRACE] = trace;
}

// yPredQuad's update (hazan.nim:167-173) and residual = y - yPredQuad (:177); part2: the workgroups' sums of the residual
__global__ void __launch_bounds__(kBlock) k_apply(const double* yt, double* ypq, double* res, const double* K, int64_t n, double eta, double* part2,
                                                  const double* sc) {
  __shared__ double red[kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double r = 0.0;
  if (i < n) {
    const double step = sc[HZ_STEP];
    double v = ypq[i] * (1 - step);
    v += eta * step * K[(int64_t)sc[HZ_S] * n + i];
    if (sc[HZ_RESCALE] != 0.0) v *= sc[HZ_SCALE];
    ypq[i] = v;
    r = yt[i] - v;
    res[i] = r;
  }
  const double s = tree_block(r, red);
  if (threadIdx.x == 0) part2[blockIdx.x] = s;
}

// ---- CG on Z^T Z, preconditioned on both sides (tensor.nim:970-1009 as hazan.nim:182-187 calls it) ----
// b[d] = sum residual (the dummy column), tol = 1e-5 * ||b||_1
__global__ void __launch_bounds__(kNarrowBlock) k_cg_bfin(const double* part_abs, int64_t np_d, const double* part_res, int64_t np_n, double* b,
                                                          int64_t d, int icpt, double* sc) {
  __shared__ double red[kNarrowBlock];
  const double mag = fin_sum(part_abs, np_d, red), sres = fin_sum(part_res, np_n, red);
  if (threadIdx.x != 0) return;
  double m = mag;
  if (icpt) {
    b[d] = sres;
    m += fabs(sres);
  }
  sc[HZ_CG_TOL] = 1e-5 * m;
  sc[HZ_CG_IT] = 0.0;
  sc[HZ_CG_STOP] = 0.0;
}

// x = w * colNormSq (hazan.nim:185), r = bPre = b / colNormSq (tensor.nim:977-979)
__global__ void __launch_bounds__(kBlock) k_cg_init0(double* x, double* r, const double* b, const double* cn, int64_t dz) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < dz) {
    x[j] *= cn[j];
    r[j] = b[j] / cn[j];
  }
}

// the dummy column's entry of Ap: (sum Xp) / colNormSq[d]
__global__ void __launch_bounds__(kNarrowBlock) k_cg_apd(const double* part_xp, int64_t np_n, double* Ap, const double* cn, int64_t d) {
  __shared__ double red[kNarrowBlock];
  const double s = fin_sum(part_xp, np_n, red);
  if (threadIdx.x == 0) Ap[d] = s / cn[d];
}

// r -= Ap; p = r (tensor.nim:987-988); part0: r . r
__global__ void __launch_bounds__(kBlock) k_cg_init2(double* r, double* p, const double* Ap, int64_t dz, double* part0) {
  __shared__ double red[kBlock];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double v = 0.0;
  if (j < dz) {
    const double rj = r[j] - Ap[j];
    r[j] = rj;
    p[j] = rj;
    v = rj * rj;
  }
  const double s = tree_block(v, red);
  if (threadIdx.x == 0) part0[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kNarrowBlock) k_cg_init3(const double* part0, int64_t np_z, double* sc) {
  __shared__ double red[kNarrowBlock];
  const double s = fin_sum(part0, np_z, red);
  if (threadIdx.x == 0) sc[HZ_CG_DOTR] = s;
}

// curv = p . Ap, alpha = dotr / curv (tensor.nim:998-999); the loop also ends when curv is 0 or not finite
__global__ void __launch_bounds__(kNarrowBlock) k_cg_curv(const double* part_xp, int64_t np_n, const double* part_pap, int64_t np_d, const double* p,
                                                          double* Ap, const double* cn, int64_t d, int icpt, double* sc) {
  __shared__ double red[kNarrowBlock];
  const bool stopped = sc[HZ_CG_STOP] != 0.0;
  __syncthreads();
  if (stopped) {
    if (threadIdx.x == 0) sc[HZ_CG_DOUPD] = 0.0;
    return;
  }
  const double sxp = fin_sum(part_xp, np_n, red);
  double curv = fin_sum(part_pap, np_d, red);
  if (threadIdx.x != 0) return;
  if (icpt) {
    Ap[d] = sxp / cn[d];
    curv += p[d] * Ap[d];
  }
  if (curv == 0.0 || !isfinite(curv)) {
    sc[HZ_CG_STOP] = 1.0;
    sc[HZ_CG_DOUPD] = 0.0;
  } else {
    sc[HZ_CG_ALPHA] = sc[HZ_CG_DOTR] / curv;
    sc[HZ_CG_DOUPD] = 1.0;
  }
}

// x += alpha p; r -= alpha Ap (tensor.nim:1000-1001); part0: r . r, part1: ||r||_1
__global__ void __launch_bounds__(kBlock) k_cg_upd(double* x, double* r, const double* p, const double* Ap, int64_t dz, double* part0, double* part1,
                                                   const double* sc) {
  __shared__ double red[kBlock];
  if (sc[HZ_CG_DOUPD] == 0.0) return;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double v = 0.0, a = 0.0;
  if (j < dz) {
    const double alpha = sc[HZ_CG_ALPHA];
    x[j] += alpha * p[j];
    const double rj = r[j] - alpha * Ap[j];
    r[j] = rj;
    v = rj * rj;
    a = fabs(rj);
  }
  const double s0 = tree_block(v, red);
  const double s1 = tree_block(a, red);
  if (threadIdx.x == 0) {
    part0[blockIdx.x] = s0;
    part1[blockIdx.x] = s1;
  }
}

// the stop on ||r||_1 < tol, else beta = dotrNew / dotr (tensor.nim:1002-1005); the cap of kCgMaxIter iterations
__global__ void __launch_bounds__(kNarrowBlock) k_cg_beta(const double* part0, const double* part1, int64_t np_z, double* sc) {
  __shared__ double red[kNarrowBlock];
  const bool upd = sc[HZ_CG_DOUPD] != 0.0;
  __syncthreads();
  if (!upd) {
    if (threadIdx.x == 0) sc[HZ_CG_DOP] = 0.0;
    return;
  }
  const double dn = fin_sum(part0, np_z, red), n1 = fin_sum(part1, np_z, red);
  if (threadIdx.x != 0) return;
  const double it = sc[HZ_CG_IT] + 1.0;
  sc[HZ_CG_IT] = it;
  if (n1 < sc[HZ_CG_TOL]) {
    sc[HZ_CG_STOP] = 1.0;
    sc[HZ_CG_DOP] = 0.0;
  } else {
    sc[HZ_CG_BETA] = dn / sc[HZ_CG_DOTR];
    sc[HZ_CG_DOTR] = dn;
    sc[HZ_CG_DOP] = 1.0;
    if (it >= (double)kCgMaxIter) sc[HZ_CG_STOP] = 1.0;
  }
}

// p = p * beta + r (tensor.nim:1006-1007)
__global__ void __launch_bounds__(kBlock) k_cg_p(double* p, const double* r, int64_t dz, const double* sc) {
  if (sc[HZ_CG_DOP] == 0.0) return;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < dz) {
    double v = p[j] * sc[HZ_CG_BETA];
    v += r[j];
    p[j] = v;
  }
}

// the closing right preconditioner (tensor.nim:1009) and the model's w and intercept (hazan.nim:189-193)
__global__ void __launch_bounds__(kBlock) k_cg_final(double* x, const double* cn, int64_t d, int64_t dz, double* w, double* msc) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < dz) {
    const double v = x[j] / cn[j];
    x[j] = v;
    if (j < d)
      w[j] = v;
    else
      msc[SC_INTERCEPT] = v;
  }
}

// the intercept alone: the residual's mean (hazan.nim:194-196)
__global__ void __launch_bounds__(kNarrowBlock) k_icpt(const double* part_res, int64_t np_n, int64_t n, double* msc) {
  __shared__ double red[kNarrowBlock];
  const double s = fin_sum(part_res, np_n, red);
  if (threadIdx.x == 0) msc[SC_INTERCEPT] = s / (double)n;
}

// residual = y - yPredQuad - yPredLinear (hazan.nim:132,201); part0: residual^2.  fill_ypl: yPredLinear = the intercept (:196)
__global__ void __launch_bounds__(kBlock) k_residual(const double* yt, const double* ypq, double* ypl, double* res, int64_t n, int fill_ypl,
                                                     const double* msc, double* part0) {
  __shared__ double red[kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    if (fill_ypl) ypl[i] = msc[SC_INTERCEPT];
    const double r = yt[i] - ypq[i] - ypl[i];
    res[i] = r;
    v = r * r;
  }
  const double s = tree_block(v, red);
  if (threadIdx.x == 0) part0[blockIdx.x] = s;
}

// norm(residual, 2)^2 / n (hazan.nim:133,202)
__global__ void __launch_bounds__(kNarrowBlock) k_loss(const double* part0, int64_t np_n, int64_t n, double* sc) {
  __shared__ double red[kNarrowBlock];
  const double s = fin_sum(part0, np_n, red);
  if (threadIdx.x == 0) {
    const double nrm = sqrt(s);
    sc[HZ_LOSS] = nrm * nrm / (double)n;
  }
}

// checkTarget (fm_base.nim:29-36); yPredQuad = 0
__global__ void __launch_bounds__(kBlock) k_targets(const double* y, int task, double* yt, double* ypq, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    yt[i] = dev::target_of(y[i], task);
    ypq[i] = 0.0;
  }
}

// colNormSq (+ nSamples for the dummy column) + 1e-5 (hazan.nim:93-99); the CG's x starts from w (+ the intercept)
__global__ void __launch_bounds__(kBlock) k_cn(double* cn, double* x, const double* w, const double* msc, int64_t d, int64_t dz, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < dz) {
    if (j < d) {
      cn[j] += 1e-5;
      x[j] = w[j];
    } else {
      cn[j] = (double)n + 1e-5;
      x[j] = msc[SC_INTERCEPT];
    }
  }
}

// ---- decisionFunction (convex_factorization_machine.nim:63-84): linear + intercept, then lams[s] * K[s] component by component ----
__global__ void __launch_bounds__(kBlock) k_cfm_predict(CsrView X, CfmView M, double* out) {
  const int g = threadIdx.x / kG, gl = threadIdx.x % kG, base = (threadIdx.x % kWave) - gl;
  const int64_t i = (int64_t)blockIdx.x * kGroups + g;
  if (i >= X.n) return;
  const int64_t q0 = X.indptr[i], q1 = X.indptr[i + 1];
  double v = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return M.w[X.indices[q]] * X.data[q]; });
  v += M.sc[SC_INTERCEPT];
  for (int s = 0; s < M.n_components; ++s) {
    const double* Ps = M.P + (int64_t)s * M.d;
    const double a1 = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) { return Ps[X.indices[q]] * X.data[q]; });
    double k;
    if (M.ignore_diag) {
      const double a2 = ordered_acc(0.0, q0, q1, gl, base, [&](int64_t q) {
        const double t = Ps[X.indices[q]] * X.data[q];
        return t * t;
      });
      k = (a1 * a1 - a2) / 2.0;
    } else {
      k = a1 * a1;
    }
    v += M.lams[s] * k;
  }
  if (gl == 0) out[i] = v;
}

// one power iteration: q = X^T (weight o (X p)) (- the diagonal), eval = <p, q>, p = q / ||q||, the stop.  weight [n]: Hazan's
// residual (hazan.nim:114-121), GreedyCD's dL (greedy_cd.nim:338-345)
void issue_power(hipStream_t st, const HazanState* S, const double* weight, int ignore_diag) {
  const Twin T = twin_of(S);
  const Lay L = layout(S);
  const Parts Pt = parts_of(S);
  double* sc = S->scal.as<double>();
  const int64_t gn = blocks_for(S->n, kGroups), gd = blocks_for(S->d, kGroups);
  HZ_LAUNCH(k_rows, gn, kBlock, T, L.pv, nullptr, nullptr, nullptr, weight, L.Xp, nullptr, sc + HZ_P_STOP);
  HZ_LAUNCH(k_cols<COL_POWER>, gd, kBlock, T, L.Xp, L.pv, weight, nullptr, ignore_diag, L.q, Pt.p0, Pt.p1, sc + HZ_P_STOP);
  HZ_LAUNCH(k_power_fin, 1, kNarrowBlock, Pt.p0, Pt.p1, gd, sc);
  HZ_LAUNCH(k_power_norm, blocks_for(S->d, kBlock), kBlock, L.q, L.pv, S->d, sc);
}

// Ap = (Z^T Z (v / cn)) / cn for the d real columns; the dummy column's entry is finished by the caller's next kernel from p2
void issue_cg_op(hipStream_t st, const HazanState* S, const double* v, const double* dotv, int icpt, const double* flag) {
  const Twin T = twin_of(S);
  const Lay L = layout(S);
  const Parts Pt = parts_of(S);
  const int64_t gn = blocks_for(S->n, kGroups), gd = blocks_for(S->d, kGroups);
  HZ_LAUNCH(k_rows, gn, kBlock, T, v, L.cn, icpt ? v + S->d : nullptr, icpt ? L.cn + S->d : nullptr, nullptr, L.Xp, Pt.p2, flag);
  HZ_LAUNCH(k_cols<COL_CG>, gd, kBlock, T, L.Xp, dotv, nullptr, L.cn, 0, L.Ap, Pt.p0, nullptr, flag);
}

void issue_cg(hipStream_t st, const HazanState* S, int icpt) {
  const Lay L = layout(S);
  const Parts Pt = parts_of(S);
  double* sc = S->scal.as<double>();
  const int64_t gn = blocks_for(S->n, kGroups), gd = blocks_for(S->d, kGroups), gz = blocks_for(S->dz, kBlock);
  issue_cg_op(st, S, L.cp, L.cp, icpt, sc + HZ_CG_STOP);
  HZ_LAUNCH(k_cg_curv, 1, kNarrowBlock, Pt.p2, gn, Pt.p0, gd, L.cp, L.Ap, L.cn, S->d, icpt, sc);
  HZ_LAUNCH(k_cg_upd, gz, kBlock, L.x, L.r, L.cp, L.Ap, S->dz, Pt.p0, Pt.p1, sc);
  HZ_LAUNCH(k_cg_beta, 1, kNarrowBlock, Pt.p0, Pt.p1, gz, sc);
  HZ_LAUNCH(k_cg_p, gz, kBlock, L.cp, L.r, S->dz, sc);
}

// kHazanChunk iterations as one graph (NFM_HAZAN_GRAPH=0: launch by launch)
template <class F>
int run_chunk(hipStream_t st, void** exec_slot, F issue) {
  static const bool use_graph = !(getenv("NFM_HAZAN_GRAPH") && atoi(getenv("NFM_HAZAN_GRAPH")) == 0);
  if (!use_graph) {
    for (int c = 0; c < kHazanChunk; ++c) issue();
    NFM_HIP_CHECK(hipGetLastError());
    return NFM_OK;
  }
  if (!*exec_slot) {
    NFM_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    for (int c = 0; c < kHazanChunk; ++c) issue();
    const hipError_t le = hipGetLastError();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (le != hipSuccess || e != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      NFM_HIP_CHECK(le);
      NFM_HIP_CHECK(e);
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    NFM_HIP_CHECK(e2);
    *exec_slot = exec;
  }
  NFM_HIP_CHECK(hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(*exec_slot), st));
  return NFM_OK;
}

int read_scalars(hipStream_t st, HazanState* S) {
  NFM_HIP_CHECK(hipMemcpyAsync(S->scal_h, S->scal.p, sizeof(double) * HZ_COUNT, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

}  // namespace

void HazanState::drop_graphs() {
  if (g_power) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(g_power));
  if (g_cg) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(g_cg));
  g_power = g_cg = nullptr;
}

HazanState::~HazanState() {
  drop_graphs();
  if (scal_h) (void)hipHostFree(scal_h);
}

int cfm_alloc(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const CfmView& M, HazanState* S, const char* who) {
  NFM_CHECK(X.n >= 1, NFM_ERR_INVALID, "nSamples < 1");
  NFM_CHECK(X.n <= (int64_t)2147483647 && X.d < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "%s: nSamples and nFeatures must fit 31 bits", who);
  S->fit_ready = false;
  S->drop_graphs();  // the captured chunks hold this fit's pointers and flags
  NFM_TRY(cd_schedule(ctx, X, uid, 0, &S->twin, nullptr, nullptr));
  hipStream_t st = ctx->stream;
  S->n = X.n;
  S->d = X.d;
  S->dz = X.d + (M.fit_intercept ? 1 : 0);
  S->maxc = M.max_components;
  NFM_TRY(S->vec.ensure(sizeof(double) * lay_doubles(S->n, S->d, S->maxc)));
  S->n_part = std::max(blocks_for(S->n, kGroups), blocks_for(S->d + 1, kGroups)) + 1;
  NFM_TRY(S->part.ensure(sizeof(double) * 4 * S->n_part));
  NFM_TRY(S->scal.ensure(sizeof(double) * HZ_COUNT));
  if (!S->scal_h) NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&S->scal_h), sizeof(double) * HZ_COUNT, hipHostMallocDefault));
  NFM_HIP_CHECK(hipMemsetAsync(S->vec.p, 0, S->vec.bytes, st));
  NFM_HIP_CHECK(hipMemsetAsync(S->part.p, 0, S->part.bytes, st));
  NFM_HIP_CHECK(hipMemsetAsync(S->scal.p, 0, S->scal.bytes, st));
  return NFM_OK;
}

int cfm_power_method(nfm_ctx* ctx, HazanState* S, const double* weight, int ignore_diag, int64_t max_iter_power, double tol_power,
                     const double* start, double* iters, double* eval) {
  hipStream_t st = ctx->stream;
  const Lay L = layout(S);
  double* sc = S->scal.as<double>();
  const int64_t d = S->d;
  // evec = start / ||start|| (tensor.nim:920-922), in order on the host
  {
    std::vector<double> p(start, start + d);
    double s = 0.0;
    for (int64_t j = 0; j < d; ++j) s += fabs(p[j]) * fabs(p[j]);
    const double nrm = sqrt(s);
    for (int64_t j = 0; j < d; ++j) p[j] /= nrm;
    NFM_HIP_CHECK(hipMemcpyAsync(L.pv, p.data(), sizeof(double) * d, hipMemcpyHostToDevice, st));
    double head[HZ_P_DONORM + 1] = {(double)max_iter_power, tol_power, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    NFM_HIP_CHECK(hipMemcpyAsync(sc, head, sizeof(head), hipMemcpyHostToDevice, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));  // p and head leave scope
  }
  *iters = 0.0;
  *eval = 0.0;
  if (max_iter_power > 0) {
    for (int64_t done = 0;; done += kHazanChunk) {
      NFM_CHECK(done < max_iter_power + kHazanChunk, NFM_ERR_HIP, "the power method's stop flag was never set");
      NFM_TRY(run_chunk(st, &S->g_power, [&] { issue_power(st, S, weight, ignore_diag); }));
      NFM_TRY(read_scalars(st, S));
      if (S->scal_h[HZ_P_STOP] != 0.0) break;
    }
    *iters = S->scal_h[HZ_P_IT];
    *eval = S->scal_h[HZ_P_EVAL];
  }
  return NFM_OK;
}

void cfm_issue_linear(nfm_ctx* ctx, const HazanState* S, const double* w, const double* intercept, double* out) {
  hipStream_t st = ctx->stream;
  HZ_LAUNCH(k_rows, blocks_for(S->n, kGroups), kBlock, twin_of(S), w, nullptr, intercept, nullptr, nullptr, out, nullptr, nullptr);
}

void cfm_issue_colsq(nfm_ctx* ctx, const HazanState* S, double* out) {
  hipStream_t st = ctx->stream;
  HZ_LAUNCH(k_cols<COL_SQ>, blocks_for(S->d, kGroups), kBlock, twin_of(S), nullptr, nullptr, nullptr, nullptr, 0, out, nullptr, nullptr, nullptr);
}

void cfm_issue_set_row(nfm_ctx* ctx, const HazanState* S, double* P, const double* slot) {
  hipStream_t st = ctx->stream;
  HZ_LAUNCH(k_set_row, blocks_for(S->d, kBlock), kBlock, P, layout(S).pv, S->d, slot);
}

int launch_cfm_predict(nfm_ctx* ctx, const CsrView& X, const CfmView& M, double* out_dev) {
  if (X.n == 0) return NFM_OK;
  TimedLaunch tl(ctx, "predict");
  hipLaunchKernelGGL(k_cfm_predict, dim3((unsigned)blocks_for(X.n, kGroups)), dim3(kBlock), 0, ctx->stream, X, M, out_dev);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

int hazan_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const CfmView& M, const HazanCfg& cfg, HazanState* S,
                    double* loss_old) {
  NFM_TRY(cfm_alloc(ctx, X, uid, M, S, "Hazan"));
  hipStream_t st = ctx->stream;
  const Twin T = twin_of(S);
  const Lay L = layout(S);
  const Parts Pt = parts_of(S);
  double* sc = S->scal.as<double>();
  const int64_t gn = blocks_for(S->n, kGroups), gd = blocks_for(S->d, kGroups), en = blocks_for(S->n, kBlock);
  HZ_LAUNCH(k_targets, en, kBlock, X.y, M.task, L.yt, L.ypq, S->n);
  HZ_LAUNCH(k_cols<COL_SQ>, gd, kBlock, T, nullptr, nullptr, nullptr, nullptr, 0, L.cn, nullptr, nullptr, nullptr);
  HZ_LAUNCH(k_cn, blocks_for(S->dz, kBlock), kBlock, L.cn, L.x, M.w, M.sc, S->d, S->dz, S->n);
  // yPredLinear = linear(X, w) + intercept (hazan.nim:102-103)
  HZ_LAUNCH(k_rows, gn, kBlock, T, M.w, nullptr, M.sc + SC_INTERCEPT, nullptr, nullptr, L.ypl, nullptr, nullptr);
  for (int s = 0; s < M.n_components; ++s)
    HZ_LAUNCH(k_kernel, gn, kBlock, T, M.P, M.lams, s, M.ignore_diag, cfg.eta, L.yt, L.ypl, L.ypq, L.res, L.K, Pt.p0, Pt.p1, sc);
  HZ_LAUNCH(k_residual, en, kBlock, L.yt, L.ypq, L.ypl, L.res, S->n, 0, M.sc, Pt.p0);
  HZ_LAUNCH(k_loss, 1, kNarrowBlock, Pt.p0, en, S->n, sc);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_scalars(st, S));
  if (loss_old) *loss_old = S->scal_h[HZ_LOSS];
  S->fit_uid = uid;
  S->fit_serial = serial;
  S->fit_ready = true;
  return NFM_OK;
}

int hazan_iter(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const HazanCfg& cfg, HazanState* S, int64_t it, const double* start,
               int32_t* n_components, double* record) {
  hipStream_t st = ctx->stream;
  const Twin T = twin_of(S);
  const Lay L = layout(S);
  const Parts Pt = parts_of(S);
  double* sc = S->scal.as<double>();
  const int64_t n = S->n, d = S->d, dz = S->dz;
  const int64_t gn = blocks_for(n, kGroups), gd = blocks_for(d, kGroups), en = blocks_for(n, kBlock), ed = blocks_for(d, kBlock),
                gz = blocks_for(dz, kBlock);
  const int icpt = M.fit_intercept ? 1 : 0;
  int nc = *n_components;

  // ---- the power method on X^T diag(residual) X ----
  double p_iters = 0.0, p_eval = 0.0;
  NFM_TRY(cfm_power_method(ctx, S, L.res, M.ignore_diag, cfg.max_iter_power, cfg.tol_power, start, &p_iters, &p_eval));

  // ---- append or replace, K[s], the residual, the step size, lams and yPredQuad (hazan.nim:144-174) ----
  HZ_LAUNCH(k_select, 1, 1, M.lams, nc, M.max_components, sc);
  if (nc < M.max_components) ++nc;
  HZ_LAUNCH(k_set_row, ed, kBlock, M.P, L.pv, d, sc + HZ_S);
  HZ_LAUNCH(k_kernel, gn, kBlock, T, M.P, M.lams, -1, M.ignore_diag, cfg.eta, L.yt, L.ypl, L.ypq, L.res, L.K, Pt.p0, Pt.p1, sc);
  HZ_LAUNCH(k_step, 1, kNarrowBlock, Pt.p0, Pt.p1, gn, M.lams, nc, cfg.eta, cfg.optimal, (double)it, sc);
  HZ_LAUNCH(k_apply, en, kBlock, L.yt, L.ypq, L.res, L.K, n, cfg.eta, Pt.p3, sc);
  NFM_HIP_CHECK(hipGetLastError());

  // ---- the linear part (hazan.nim:176-196) ----
  double cg_iters = 0.0;
  int fill_ypl = 0;
  if (M.fit_linear) {
    HZ_LAUNCH(k_cols<COL_B>, gd, kBlock, T, L.res, nullptr, nullptr, nullptr, 0, L.b, Pt.p0, nullptr, nullptr);
    HZ_LAUNCH(k_cg_bfin, 1, kNarrowBlock, Pt.p0, gd, Pt.p3, en, L.b, d, icpt, sc);
    HZ_LAUNCH(k_cg_init0, gz, kBlock, L.x, L.r, L.b, L.cn, dz);
    issue_cg_op(st, S, L.x, L.r, icpt, nullptr);
    if (icpt) HZ_LAUNCH(k_cg_apd, 1, kNarrowBlock, Pt.p2, gn, L.Ap, L.cn, d);
    HZ_LAUNCH(k_cg_init2, gz, kBlock, L.r, L.cp, L.Ap, dz, Pt.p0);
    HZ_LAUNCH(k_cg_init3, 1, kNarrowBlock, Pt.p0, gz, sc);
    NFM_HIP_CHECK(hipGetLastError());
    for (int64_t done = 0;; done += kHazanChunk) {
      NFM_CHECK(done < kCgMaxIter + kHazanChunk, NFM_ERR_HIP, "Hazan: the conjugate gradient's stop flag was never set");
      NFM_TRY(run_chunk(st, &S->g_cg, [&] { issue_cg(st, S, icpt); }));
      NFM_TRY(read_scalars(st, S));
      if (S->scal_h[HZ_CG_STOP] != 0.0) break;
    }
    cg_iters = S->scal_h[HZ_CG_IT];
    HZ_LAUNCH(k_cg_final, gz, kBlock, L.x, L.cn, d, dz, M.w, M.sc);
    HZ_LAUNCH(k_rows, gn, kBlock, T, L.x, nullptr, icpt ? L.x + d : nullptr, nullptr, nullptr, L.ypl, nullptr, nullptr);
  } else if (icpt) {
    HZ_LAUNCH(k_icpt, 1, kNarrowBlock, Pt.p3, en, n, M.sc);
    fill_ypl = 1;
  }
  HZ_LAUNCH(k_residual, en, kBlock, L.yt, L.ypq, L.ypl, L.res, n, fill_ypl, M.sc, Pt.p0);
  HZ_LAUNCH(k_loss, 1, kNarrowBlock, Pt.p0, en, n, sc);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_scalars(st, S));
  *n_components = nc;
  const double* h = S->scal_h;
  record[NFM_HAZAN_REC_LOSS] = h[HZ_LOSS];
  record[NFM_HAZAN_REC_TRACE] = h[HZ_TRACE];
  record[NFM_HAZAN_REC_SLOT] = h[HZ_S];
  record[NFM_HAZAN_REC_STEP] = h[HZ_STEP];
  record[NFM_HAZAN_REC_POWER_ITERS] = p_iters;
  record[NFM_HAZAN_REC_CG_ITERS] = cg_iters;
  record[NFM_HAZAN_REC_EVAL] = p_eval;
  record[NFM_HAZAN_REC_N_COMPONENTS] = (double)nc;
  (void)X;
  return NFM_OK;
}

}  // namespace nfm
