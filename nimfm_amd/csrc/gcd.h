// nimfm_amd/csrc/gcd.h -- greedy coordinate descent for the convex factorization machine (optimizer/greedy_cd.nim at
// refitFully = false) on the device: the per-optimizer state of gcd.hip.
#pragma once
#include "cfm.h"

namespace nfm {

struct GcdCfg {  // newGreedyCD (greedy_cd.nim:25-30); maxIter, maxIterInner, nRefitting, tol and verbose stay with the host loop
  double alpha0, alpha, beta;  // as the caller gave them; the solver steps scale them by nSamples (:424-426)
  int32_t loss;
  double loss_param;
  int64_t max_iter_power;
  double tol_power;
  int32_t refit_fully;  // refused at begin_fit: ADMM, Newton-CG and two dsyev calls stay with the reference
};

struct GcdState {
  HazanState core;  // the twin with its levels, the vectors over n and d, K, the partial sums, the power method's scalars and chunk
  DevBuf gsc;       // GreedyCD's device scalars (G_*)
  DevBuf out;       // [1 + d]: |update| of the intercept step and of the w sweep (cd.hip's kernels write it)
  double* gsc_h = nullptr;  // pinned copy of gsc
  int32_t nc_nonzero = 0;   // the count of non-zero lams the last step reported: whether the next inner step adds a base
  bool outer_open = false;  // between nfm_gcd_outer_begin and nfm_gcd_outer_end
  ~GcdState();
};

// greedy_cd.nim:419-457: the twin and the levels, colNormSq, yPred = linear + intercept + sum lams[s] K[s] with K rebuilt from
// the components the model holds; *loss_old, *reg_old are :455-457's
int gcd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const CfmView& M, const GcdCfg& cfg, GcdState* S,
                  double* loss_old, double* reg_old);
// :464-469 and fitZ's head :332-336: fitInterceptCD, fitLinearCD, nComponents and the old inner objective
int gcd_outer_begin(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, double* record);
// :347-397, one inner iteration: with `start` (host, d doubles) dL, the power method, the slot, K[s], fitLams and yPred; with
// `refit` refitDiag; then the inner objective.  *n_components is the model's count of stored components before and after.
int gcd_inner(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, const double* start, int refit,
              int32_t* n_components, double* record);
// :474-476 and, with `recompute`, :493-497
int gcd_outer_end(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const GcdCfg& cfg, GcdState* S, int recompute, double* loss, double* reg);

}  // namespace nfm
