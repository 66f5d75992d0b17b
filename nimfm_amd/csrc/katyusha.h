// nimfm_amd/csrc/katyusha.h -- Katyusha (optimizer/katyusha.nim) with its seven parameter sets resident on the device
// (katyusha.hip).
#pragma once
#include <memory>
#include <vector>

#include "pgd.h"

namespace nfm {

struct KatCfg {
  double eta = 0.1, alpha0 = 1e-6, alpha = 1e-3, beta = 1e-4, gamma = 1e-4;
  double tau1 = 0.5, tau2 = -1.0;  // as the user gave them: negative = derived in kat_begin_fit (katyusha.nim:208-213)
  int32_t loss = 0;
  double loss_param = 1.0;
  int32_t reg = NFM_REG_SQUAREDL12, reg_transpose = 1;
  int64_t batch = 1;  // miniBatchSize, resolved by the host
};

struct KatState {
  KatCfg cfg;
  // ---- one fit (nothing is carried between fits: katyusha.nim:182-216 starts every fit from the model alone) ----
  bool fit_ready = false;
  uint64_t fit_uid = 0, fit_serial = 0;
  int64_t n = 0, m_inner = 0;  // maxIterInner
  double tau1 = 0, tau2 = 0;   // the fit's own values
  bool grad_stale = false;     // tilde moved since grads_ave was taken: the next epoch call starts with predictAllWithGrad(tilde)
  double loss_sum = 0;         // sum_i loss(y_i, yPred_i) of the last predictAllWithGrad
  PgdSet x, z, y, tilde, next, gave;  // params, z_params, y_params, tilde_params, next_tilde_params, grads_ave
  PgdSet gx, gt;                      // the mini-batch gradient at params and at tilde_params (rows of touched features only)
  DevBuf stamp;                       // int32[da]: the inner iteration that last touched a feature
  int32_t stamp_cur = 0;
  DevBuf prox, partial, rec;
  double* pin = nullptr;  // pinned: {loss_sum, -} of a gradient pass, then the epoch's record
  std::unique_ptr<Plan> gplan, plan;  // the one-batch plan of the dataset; the plan of the epoch's index stream
  MbWork Wg, W;
  std::vector<int64_t> ident;  // perm == NULL: the identity stream with wrap-around
  ~KatState();
};

// katyusha.nim:182-219: the sets, y, z, tilde <- params, maxIterInner, tau1, tau2, the first predictAllWithGrad
int kat_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, KatState* S);
// one outer iteration (katyusha.nim:229-262) over the index stream perm[begin .. end)
int kat_epoch(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const ModelView& M, KatState* S, const int64_t* perm, int64_t begin,
              int64_t end, double* loss_sum, double* viol_sum);

}  // namespace nfm
