// nimfm_amd/csrc/pgd.h -- the full-batch proximal gradient solvers PGD, FISTA and NMAPGD (optimizer/pgd.nim, fista.nim,
// nmapgd.nim) with parameters, gradients and line-search state resident on the device (pgd.hip).
#pragma once
#include <memory>

#include "mb.h"

namespace nfm {

// one parameter set of model/params.nim: P in the device block layout, w, and the scalars (sc[SC_INTERCEPT]; both scales 1)
struct PgdSet {
  DevBuf buf;
  size_t bP = 0, bw = 0;
  double* P() const { return buf.as<double>(); }
  double* w() const { return reinterpret_cast<double*>(buf.as<char>() + bP); }
  double* sc() const { return reinterpret_cast<double*>(buf.as<char>() + bP + bw); }
};

// a record slot of the reduction passes: {b_new, dot_b, viol_b, loss_sum}, then the sums of k_pgd_finish
enum { RS_B = 0, RS_DOTB = 1, RS_VIOLB = 2, RS_LOSS = 3, RS_PART = 4 };
constexpr int kPgdMaxBlocks = 1024;  // workgroups per device block of a reduction pass (the finish adds that many partials)

struct PgdCfg {
  int32_t algo = NFM_PGD_ALGO_PGD;
  double alpha0 = 0, alpha = 0, beta = 0, gamma = 0, rho = 0.5, sigma = 1.0, eta = 0.5;
  int32_t loss = 0;
  double loss_param = 1.0;
  int32_t reg = NFM_REG_SQUAREDL12, reg_transpose = 1;
  int64_t max_search = -1;
};

// what nfm_pgd_last_iter reports (the NFM_PGD_IT_* slots of include/nimfm_hip.h)
struct PgdIter {
  double lossVal = 0, regVal = 0, viol = 0;
  double eta[2] = {0, 0};      // the line search's step size when it ended (NMAPGD: Z, then V)
  double start[2] = {0, 0};    // the step size it started from (PGD, FISTA: 1; NMAPGD: getStepSize)
  double trials[2] = {0, 0};   // trials of each line search (0: not run)
  double branch = 0;           // NFM_PGD_BRANCH_*
  double t = 0, c = 0, q = 0;  // the optimizer's t (FISTA, NMAPGD), NMAPGD's c and q after the iteration
};

struct PgdState {
  PgdCfg cfg;
  // ---- one fit ----
  bool fit_ready = false;
  uint64_t fit_uid = 0, fit_serial = 0;
  int64_t n = 0;
  PgdSet old, grads;                                  // PGD, FISTA: old_params; all: the gradient of the current point
  PgdSet z;                                           // FISTA: z_params; NMAPGD: self.z_params
  PgdSet y, old_x, old_y, old_y_grads, x_grads;       // NMAPGD
  int64_t shape_key = -1;                             // (nb, da, Kp, d) the sets were allocated for
  DevBuf yhat, partial, colpart, lpart, prox, rec;
  double* rec_h = nullptr;                            // pinned copy of `rec`
  int slot = 0;                                       // doubles per record slot
  // ---- carried between iterations (and between warm-started fits) ----
  double t = 0.0, c = -1.0, q = 1.0;
  double lossVal = 0.0, regVal = 0.0;                 // FISTA: the accepted objective of this fit
  PgdIter last;
  // the one-batch plan of the dataset and the scratch of the gradient's row / column phase
  std::unique_ptr<Plan> plan;
  MbWork W;
  ~PgdState();
};

// pgd.predictAllWithGrad (optimizer/pgd.nim:70-103) of the parameters M points at, into device buffers in the layout of a
// parameter set (gP must be zeroed by the caller: features no sample touches keep a zero gradient).  plan / W: the one-batch
// plan of the dataset (built on first use, kept) and its scratch.  out2_host[0] = sum_i loss(y_i, yPred_i).
int full_gradient(nfm_ctx* ctx, const CsrView& X, uint64_t ds_uid, const ModelView& M, const OptView& O, std::unique_ptr<Plan>& plan,
                  MbWork& W, double* gP, double* gw, double* gb, int64_t it, double* out2_host);

int pgd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, bool warm_start, PgdState* S);
// one iteration of pgd.nim:186-211 / fista.nim:99-135 / nmapgd.nim:221-263, line search included
int pgd_epoch(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const ModelView& M, PgdState* S, double* loss_sum, double* viol_sum);

// a parameter set for M's shape (zero: cleared, both scales 1)
int pgd_alloc_set(nfm_ctx* ctx, const ModelView& M, PgdSet& s, bool zero);
// k_pgd_mix: dst <- A; (scale_first: dst *= ca;) dst.add(B, cb); dst.add(C, cc) per element in that order, the linear term and
// the intercept gated as params.nim:41-48,61-66 gate them.  Sets by their three device pointers {P, w, sc}.
struct PgdRef {
  double *P, *w, *sc;
};
int launch_pgd_mix(nfm_ctx* ctx, const ModelView& M, PgdRef dst, PgdRef A, PgdRef B, PgdRef C, bool scale_first, double ca, double cb, double cc);
// k_pgd_finish: partial[NY][G][4] added in workgroup order into rec[RS_PART + 4 * y + q]
int launch_pgd_finish(nfm_ctx* ctx, const double* partial, int NY, int G, double* rec);

// psgd.hip: the column-coupled proximal operators on M.P with an explicit lam (column-wise SquaredL12: threshold passes and
// apply; SquaredL21: the vector operator on `prox`'s row norms, then the rescale).  prox: MbWork::prox's layout.
void launch_prox_coupled(nfm_ctx* ctx, const ModelView& M, int reg, double lam, double* prox);
size_t prox_scratch_doubles(const ModelView& M);

}  // namespace nfm
