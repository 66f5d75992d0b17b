// nimfm_amd/csrc/gcd.hip -- greedy coordinate descent for the convex factorization machine (optimizer/greedy_cd.nim:76-109,
// 320-500 at refitFully = false) for gfx950.
//
// yPred, dL, K [maxComponents][n], P, lams, w, colNormSq and the power method's vectors stay on the device; the host loop owns
// the control flow and gets one small record per step.  The passes are cfm.hip's (the power method on X^T diag(dL) X, the row
// pass behind K[s], linear(X, w), colNormSq) and cd.hip's (fitInterceptCD, and fitLinearCD as the level sweep over the twin);
// this file adds dL, fitLams, the yPred updates, refitDiag and the objective sums.  Everything is fp64; sums over n or d are
// the fixed trees of cfm_dev.h, nothing is atomic, two runs give the same bits.  No kernel here is captured in a graph: the
// only graph of a fit is the power method's chunk.
#include <math.h>

#include <algorithm>

#include "cfm_dev.h"
#include "gcd.h"

namespace nfm {
namespace {

enum { G_SLOT = 0, G_OLD, G_NEW, G_SKIP, G_ADDED, G_NC, G_OBJ, G_LOSS, G_REG, G_NORM1, G_COUNT = 16 };

struct LossDev {
  const double* y;
  int32_t task, loss;
  double lp;
};

// dL = dloss(y, yPred) (greedy_cd.nim:352-353, :103-104).  With a component s >= 0 (refitDiag) nothing happens when lams[s] is
// zero, and part0 / part1 get the workgroups' sums of dL * K[s] and K[s]^2 that fitLams needs (:83-85)
__global__ void __launch_bounds__(kBlock) k_gcd_dl(LossDev Ld, const double* yp, double* dL, const double* K, const double* lams, int s, int64_t n,
                                                   double* part0, double* part1) {
  __shared__ double red[kBlock];
  if (s >= 0 && lams[s] == 0.0) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double a = 0.0, b = 0.0;
  if (i < n) {
    const double dl = dev::loss_grad(Ld.loss, Ld.lp, dev::target_of(Ld.y[i], Ld.task), yp[i]);
    dL[i] = dl;
    if (s >= 0) {
      const double k = K[(int64_t)s * n + i];
      a = dl * k;
      b = k * k;
    }
  }
  if (s >= 0) {
    const double s0 = tree_block(a, red);
    const double s1 = tree_block(b, red);
    if (threadIdx.x == 0) {
      part0[blockIdx.x] = s0;
      part1[blockIdx.x] = s1;
    }
  }
}

// the slot of the new basis vector (greedy_cd.nim:357-364): the first s with lams[s] == 0, else appended
__global__ void k_gcd_select(double* lams, int len, int maxc, double* gsc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int s = len;
  for (int t = 0; t < len; ++t)
    if (lams[t] == 0.0) {
      s = t;
      break;
    }
  if (s >= maxc) s = maxc - 1;  // never reached: the host adds a base only while fewer than maxComponents lams are non-zero
  if (s == len) lams[s] = 0.0;
  gsc[G_SLOT] = (double)s;
}

// K[s] of one component (cfm_dev.h's kernel_value).  init (begin_fit, s = s_fixed): yPred += lams[s] * K[s] (:449-452).  else (s
// from gsc): part0 / part1 get the workgroups' sums of dL * K[s] and K[s]^2 (fitLams, :83-85)
__global__ void __launch_bounds__(kBlock) k_gcd_kernel(Twin T, const double* P, const double* lams, int s_fixed, const double* gsc, int ignore_diag,
                                                       const double* dL, double* yp, double* K, double* part0, double* part1) {
  __shared__ double red[kGroups], red2[kGroups];
  const bool init = s_fixed >= 0;
  const int s = init ? s_fixed : (int)gsc[G_SLOT];
  const int g = threadIdx.x / kG, gl = threadIdx.x % kG, base = (threadIdx.x % kWave) - gl;
  const int64_t i = (int64_t)blockIdx.x * kGroups + g;
  const double* Ps = P + (int64_t)s * T.d;
  double a = 0.0, b = 0.0;
  if (i < T.n) {
    const double k = kernel_value(T.ridx, T.rval, Ps, T.rptr[i], T.rptr[i + 1], gl, base, ignore_diag);
    if (gl == 0) {
      K[(int64_t)s * T.n + i] = k;
      if (init) {
        yp[i] += lams[s] * k;
      } else {
        a = dL[i] * k;
        b = k * k;
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

// fitLams (greedy_cd.nim:76-94) of one slot: invStepSize = mu * sum K[s]^2 with no guard, the three-way soft threshold as
// written (a NaN falls to its last branch).  Leaves the old and the new value and a skip flag for the yPred update: refit
// (refitDiag, :101-109) skips a slot whose lams is zero on entry; a new base (:377-381) skips when the new value is zero, and
// counts itself otherwise.
__global__ void __launch_bounds__(kNarrowBlock) k_gcd_fitlams(const double* part0, const double* part1, int64_t np, double* lams, int s_fixed,
                                                              double bn, double mu, int refit, double* gsc) {
  __shared__ double red[kNarrowBlock];
  const int s = s_fixed >= 0 ? s_fixed : (int)gsc[G_SLOT];
  const double old = lams[s];
  __syncthreads();
  if (refit && old == 0.0) {
    if (threadIdx.x == 0) gsc[G_SKIP] = 1.0;
    return;
  }
  const double update = fin_sum(part0, np, red), norm = fin_sum(part1, np, red);
  if (threadIdx.x != 0) return;
  const double inv = mu * norm;
  double l = old - update / inv;
  if ((l - bn / inv) > 0)
    l -= bn / inv;
  else if ((l + bn / inv) < 0)
    l += bn / inv;
  else
    l = 0.0;
  lams[s] = l;
  gsc[G_OLD] = old;
  gsc[G_NEW] = l;
  if (refit) {
    gsc[G_SKIP] = 0.0;
  } else {
    gsc[G_SKIP] = l != 0.0 ? 0.0 : 1.0;
    gsc[G_ADDED] = l != 0.0 ? 1.0 : 0.0;
  }
}

// a new base: yPred += lams[s] * K[s] (:379); refit: yPred -= old * K[s], then yPred += new * K[s] (:107-108, two roundings)
__global__ void __launch_bounds__(kBlock) k_gcd_update(double* yp, const double* K, int s_fixed, int64_t n, int refit, const double* gsc) {
  if (gsc[G_SKIP] != 0.0) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int s = s_fixed >= 0 ? s_fixed : (int)gsc[G_SLOT];
  const double k = K[(int64_t)s * n + i];
  double v = yp[i];
  if (refit) v -= gsc[G_OLD] * k;
  v += gsc[G_NEW] * k;
  yp[i] = v;
}

// the workgroups' sums of loss(y, yPred)
__global__ void __launch_bounds__(kBlock) k_gcd_loss(LossDev Ld, const double* yp, int64_t n, double* part0) {
  __shared__ double red[kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double v = i < n ? dev::loss_value(Ld.loss, Ld.lp, dev::target_of(Ld.y[i], Ld.task), yp[i]) : 0.0;
  const double s = tree_block(v, red);
  if (threadIdx.x == 0) part0[blockIdx.x] = s;
}

// the workgroups' sums of |w|^2 (norm(w, 2), utils.nim:58)
__global__ void __launch_bounds__(kBlock) k_gcd_wsq(const double* w, int64_t d, double* part1) {
  __shared__ double red[kBlock];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double v = j < d ? fabs(w[j]) * fabs(w[j]) : 0.0;
  const double s = tree_block(v, red);
  if (threadIdx.x == 0) part1[blockIdx.x] = s;
}

// the objectives.  fitZ's (:332-336, :394-397): (sum loss + beta n ||lams||_1) / n, and the count of non-zero lams.  With
// np_d >= 0 the outer one too (:455-457, :474-476): loss = sum loss / n, reg = 0.5 alpha0 b^2 + 0.5 alpha norm(w, 2)^2 + beta
// ||lams||_1 with the unscaled strengths (the term of P has beta = 0)
__global__ void __launch_bounds__(kNarrowBlock) k_gcd_obj(const double* part0, int64_t np_n, const double* part1, int64_t np_d, const double* lams,
                                                          int len, double bn, int64_t n, double alpha0, double alpha, double beta, const double* msc,
                                                          double* gsc) {
  __shared__ double red[kNarrowBlock];
  const double S = fin_sum(part0, np_n, red);
  const double wsq = np_d >= 0 ? fin_sum(part1, np_d, red) : 0.0;
  if (threadIdx.x != 0) return;
  double norm1 = 0.0;
  int nc = 0;
  for (int t = 0; t < len; ++t) {
    norm1 += fabs(lams[t]);
    if (lams[t] != 0.0) ++nc;
  }
  gsc[G_NC] = (double)nc;
  gsc[G_NORM1] = norm1;
  gsc[G_OBJ] = (norm1 * bn + S) / (double)n;
  if (np_d >= 0) {
    const double b = msc[SC_INTERCEPT], nrm = sqrt(wsq);
    double reg = 0.5 * alpha0 * (b * b) + 0.5 * alpha * (nrm * nrm);
    reg += beta * norm1;
    gsc[G_LOSS] = S / (double)n;
    gsc[G_REG] = reg;
  }
}

// yPred (= linear + intercept on entry) += lams[s] * K[s], components in ascending s (:496-497)
__global__ void __launch_bounds__(kBlock) k_gcd_rebuild(double* yp, const double* K, const double* lams, int len, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double v = yp[i];
  for (int s = 0; s < len; ++s) v += lams[s] * K[(int64_t)s * n + i];
  yp[i] = v;
}

LossDev loss_of(const CsrView& X, const CfmView& M, const GcdCfg& cfg) { return LossDev{X.y, M.task, cfg.loss, cfg.loss_param}; }

int read_gsc(hipStream_t st, GcdState* S) {
  NFM_HIP_CHECK(hipMemcpyAsync(S->gsc_h, S->gsc.p, sizeof(double) * G_COUNT, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

// sum loss, ||lams||_1, the count and (outer) norm(w, 2): the objective's launches
void issue_objective(hipStream_t st, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, int len, bool outer) {
  const HazanState* H = &S->core;
  const Lay L = layout(H);
  const Parts Pt = parts_of(H);
  const int64_t n = H->n, d = H->d, en = blocks_for(n, kBlock), ed = blocks_for(d, kBlock);
  HZ_LAUNCH(k_gcd_loss, en, kBlock, loss_of(X, M, cfg), L.ypq, n, Pt.p0);
  if (outer) HZ_LAUNCH(k_gcd_wsq, ed, kBlock, M.w, d, Pt.p1);
  HZ_LAUNCH(k_gcd_obj, 1, kNarrowBlock, Pt.p0, en, Pt.p1, outer ? ed : (int64_t)-1, M.lams, len, cfg.beta * (double)n, n, cfg.alpha0, cfg.alpha,
            cfg.beta, M.sc, S->gsc.as<double>());
}

}  // namespace

GcdState::~GcdState() {
  if (gsc_h) (void)hipHostFree(gsc_h);
}

int gcd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const CfmView& M, const GcdCfg& cfg, GcdState* S,
                  double* loss_old, double* reg_old) {
  NFM_CHECK(!cfg.refit_fully, NFM_ERR_UNSUPPORTED,
            "GreedyCD: refitFully = true (ADMM, Newton-CG and LAPACK's dsyev) stays with the reference; refitFully = false runs here");
  HazanState* H = &S->core;
  NFM_TRY(cfm_alloc(ctx, X, uid, M, H, "GreedyCD"));
  hipStream_t st = ctx->stream;
  S->outer_open = false;
  NFM_TRY(S->gsc.ensure(sizeof(double) * G_COUNT));
  NFM_TRY(S->out.ensure(sizeof(double) * (size_t)(1 + H->d)));
  if (!S->gsc_h) NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&S->gsc_h), sizeof(double) * G_COUNT, hipHostMallocDefault));
  NFM_HIP_CHECK(hipMemsetAsync(S->gsc.p, 0, S->gsc.bytes, st));
  NFM_HIP_CHECK(hipMemsetAsync(S->out.p, 0, S->out.bytes, st));
  const Twin T = twin_of(H);
  const Lay L = layout(H);
  const Parts Pt = parts_of(H);
  const int64_t gn = blocks_for(H->n, kGroups);
  if (M.fit_linear) cfm_issue_colsq(ctx, H, L.cn);
  cfm_issue_linear(ctx, H, M.w, M.sc + SC_INTERCEPT, L.ypq);
  for (int s = 0; s < M.n_components; ++s)
    HZ_LAUNCH(k_gcd_kernel, gn, kBlock, T, M.P, M.lams, s, S->gsc.as<double>(), M.ignore_diag, L.res, L.ypq, L.K, Pt.p0, Pt.p1);
  issue_objective(st, X, M, cfg, S, M.n_components, true);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_gsc(st, S));
  if (loss_old) *loss_old = S->gsc_h[G_LOSS];
  if (reg_old) *reg_old = S->gsc_h[G_REG];
  S->nc_nonzero = (int32_t)S->gsc_h[G_NC];
  H->fit_uid = uid;
  H->fit_serial = serial;
  H->fit_ready = true;
  return NFM_OK;
}

int gcd_outer_begin(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, double* record) {
  HazanState* H = &S->core;
  hipStream_t st = ctx->stream;
  const Twin T = twin_of(H);
  const Lay L = layout(H);
  const double nd = (double)H->n;
  CdDev D{};
  D.rptr = T.rptr; D.ridx = T.ridx; D.rval = T.rval; D.cptr = T.cptr; D.crow = T.crow; D.cval = T.cval;
  D.y = X.y; D.yp = L.ypq; D.colsq = L.cn; D.out = S->out.as<double>(); D.w = M.w; D.sc = M.sc;
  D.n = H->n; D.d = H->d; D.task = M.task; D.loss = cfg.loss; D.A_ld = 3;
  D.lp = cfg.loss_param; D.mu = cd_loss_mu(cfg.loss); D.a0n = cfg.alpha0 * nd; D.an = cfg.alpha * nd; D.bn = cfg.beta * nd;
  if (M.fit_intercept) NFM_TRY(cd_issue_intercept(ctx, D));
  if (M.fit_linear) NFM_TRY(cd_issue_linear(ctx, D, &H->twin));
  issue_objective(st, X, M, cfg, S, M.n_components, false);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_gsc(st, S));
  S->nc_nonzero = (int32_t)S->gsc_h[G_NC];
  for (int t = 0; t < NFM_GCD_REC_COUNT; ++t) record[t] = 0.0;
  record[NFM_GCD_REC_SLOT] = -1.0;
  record[NFM_GCD_REC_N_COMPONENTS] = S->gsc_h[G_NC];
  record[NFM_GCD_REC_OBJECTIVE] = S->gsc_h[G_OBJ];
  record[NFM_GCD_REC_N_STORED] = (double)M.n_components;
  return NFM_OK;
}

int gcd_inner(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, const double* start, int refit,
              int32_t* n_components, double* record) {
  HazanState* H = &S->core;
  hipStream_t st = ctx->stream;
  const Twin T = twin_of(H);
  const Lay L = layout(H);
  const Parts Pt = parts_of(H);
  double* gsc = S->gsc.as<double>();
  const int64_t n = H->n, gn = blocks_for(n, kGroups), en = blocks_for(n, kBlock);
  const LossDev Ld = loss_of(X, M, cfg);
  const double bn = cfg.beta * (double)n, mu = cd_loss_mu(cfg.loss);
  int len = *n_components;
  double p_iters = 0.0, p_eval = 0.0, added = 0.0, slot = -1.0, lam = 0.0;

  if (start) {  // a new basis vector: the dominant eigenvector of X^T diag(dL) X (greedy_cd.nim:350-381)
    HZ_LAUNCH(k_gcd_dl, en, kBlock, Ld, L.ypq, L.res, L.K, M.lams, -1, n, Pt.p0, Pt.p1);
    NFM_HIP_CHECK(hipGetLastError());
    NFM_TRY(cfm_power_method(ctx, H, L.res, M.ignore_diag, cfg.max_iter_power, cfg.tol_power, start, &p_iters, &p_eval));
    HZ_LAUNCH(k_gcd_select, 1, 1, M.lams, len, M.max_components, gsc);
    cfm_issue_set_row(ctx, H, M.P, gsc + G_SLOT);
    HZ_LAUNCH(k_gcd_kernel, gn, kBlock, T, M.P, M.lams, -1, gsc, M.ignore_diag, L.res, L.ypq, L.K, Pt.p0, Pt.p1);
    HZ_LAUNCH(k_gcd_fitlams, 1, kNarrowBlock, Pt.p0, Pt.p1, gn, M.lams, -1, bn, mu, 0, gsc);
    HZ_LAUNCH(k_gcd_update, en, kBlock, L.ypq, L.K, -1, n, 0, gsc);
    NFM_HIP_CHECK(hipGetLastError());
    NFM_TRY(read_gsc(st, S));  // the slot: whether the model's stored count grew
    slot = S->gsc_h[G_SLOT];
    lam = S->gsc_h[G_NEW];
    added = S->gsc_h[G_ADDED];
    if ((int)slot == len) ++len;
  }
  if (refit) {  // refitDiag (:97-109): per stored component dL, fitLams, the two yPred updates; the device skips a zero lams[s]
    for (int s = 0; s < len; ++s) {
      HZ_LAUNCH(k_gcd_dl, en, kBlock, Ld, L.ypq, L.res, L.K, M.lams, s, n, Pt.p0, Pt.p1);
      HZ_LAUNCH(k_gcd_fitlams, 1, kNarrowBlock, Pt.p0, Pt.p1, en, M.lams, s, bn, mu, 1, gsc);
      HZ_LAUNCH(k_gcd_update, en, kBlock, L.ypq, L.K, s, n, 1, gsc);
    }
  }
  issue_objective(st, X, M, cfg, S, len, false);
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_gsc(st, S));
  S->nc_nonzero = (int32_t)S->gsc_h[G_NC];
  *n_components = len;
  record[NFM_GCD_REC_ADDED] = added;
  record[NFM_GCD_REC_SLOT] = slot;
  record[NFM_GCD_REC_LAM] = lam;
  record[NFM_GCD_REC_POWER_ITERS] = p_iters;
  record[NFM_GCD_REC_EVAL] = p_eval;
  record[NFM_GCD_REC_N_COMPONENTS] = S->gsc_h[G_NC];
  record[NFM_GCD_REC_OBJECTIVE] = S->gsc_h[G_OBJ];
  record[NFM_GCD_REC_N_STORED] = (double)len;
  return NFM_OK;
}

int gcd_outer_end(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, int recompute, double* loss, double* reg) {
  HazanState* H = &S->core;
  hipStream_t st = ctx->stream;
  const Lay L = layout(H);
  issue_objective(st, X, M, cfg, S, M.n_components, true);
  if (recompute) {
    cfm_issue_linear(ctx, H, M.w, M.sc + SC_INTERCEPT, L.ypq);
    HZ_LAUNCH(k_gcd_rebuild, blocks_for(H->n, kBlock), kBlock, L.ypq, L.K, M.lams, M.n_components, H->n);
  }
  NFM_HIP_CHECK(hipGetLastError());
  NFM_TRY(read_gsc(st, S));
  if (loss) *loss = S->gsc_h[G_LOSS];
  if (reg) *reg = S->gsc_h[G_REG];
  return NFM_OK;
}

}  // namespace nfm
