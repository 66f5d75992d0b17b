// nimfm_amd/csrc/cfm.h -- the convex factorization machine (model/convex_factorization_machine.nim) and Hazan's algorithm
// (optimizer/hazan.nim) on the device: the model's buffers and the per-optimizer state of cfm.hip.
#pragma once
#include "cd.h"

namespace nfm {

// the convex model on the device: P [max_components][d] row-major (the reference's layout), lams [max_components]; w and the
// intercept live where every model keeps them (ModelView::w, sc[SC_INTERCEPT])
struct CfmView {
  double* P;
  double* lams;
  double* w;
  double* sc;
  int64_t d;
  int32_t max_components, n_components, ignore_diag, fit_linear, fit_intercept, task;
};

struct HazanCfg {  // newHazan (hazan.nim:22-46); maxIter, tol, nTol and verbose stay with the host loop
  double eta, tol_power;
  int64_t max_iter_power;
  int32_t optimal;
};

// what one outer iteration hands the host (nfm_hazan_iter's record, NFM_HAZAN_REC_*)
constexpr int kHazanRec = NFM_HAZAN_REC_COUNT;
constexpr int kCgMaxIter = 1000;  // the reference's loop has no working cap (tensor.nim:992 never increments `it`)
constexpr int kHazanChunk = 32;   // power / CG iterations captured as one graph

struct HazanState {
  CdState twin;  // rows with ascending column ids and the column twin (cd_schedule's builder; its levels are not used)
  uint64_t fit_uid = 0, fit_serial = 0;
  bool fit_ready = false;
  int64_t n = 0, d = 0, dz = 0;
  int32_t maxc = 0;
  DevBuf vec;      // one allocation, cut by layout(): the vectors over n, over d + 1 and K
  DevBuf part;     // partial sums: [4][n_part]
  DevBuf scal;     // device scalars (HZ_*), flags
  int64_t n_part = 0;
  double* scal_h = nullptr;  // pinned copy of scal
  void* g_power = nullptr;   // graphs of kHazanChunk iterations
  void* g_cg = nullptr;
  void drop_graphs();
  ~HazanState();
};

int launch_cfm_predict(nfm_ctx* ctx, const CsrView& X, const CfmView& M, double* out_dev);

// ---- what Hazan and GreedyCD (gcd.h) both run; the kernels are cfm.hip's ----
// the twin of the dataset (with its levels), vec / part / scal sized for (n, d, max_components) and zeroed; `who` names the
// solver in the error text
int cfm_alloc(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const CfmView& M, HazanState* S, const char* who);
// powerMethod (tensor.nim:912-934) on X^T diag(weight) X (minus the diagonal with ignore_diag): weight [n] on the device
// (Hazan: the residual, hazan.nim:114-121; GreedyCD: dL, greedy_cd.nim:338-345; one pointer per fit: the captured chunk holds
// it), start [d] on the host, not normalised.  The eigenvector is left in layout(S).pv; *iters is the reference's count.
int cfm_power_method(nfm_ctx* ctx, HazanState* S, const double* weight, int ignore_diag, int64_t max_iter_power, double tol_power,
                     const double* start, double* iters, double* eval);
// out[i] = linear(X, w)[i] (+ 1.0 * *intercept when given)
void cfm_issue_linear(nfm_ctx* ctx, const HazanState* S, const double* w, const double* intercept, double* out);
// out[j] = norm(X, 2, axis = 0)[j]^2
void cfm_issue_colsq(nfm_ctx* ctx, const HazanState* S, double* out);
// P[*slot] = the power method's vector
void cfm_issue_set_row(nfm_ctx* ctx, const HazanState* S, double* P, const double* slot);
// hazan.nim:59-134: the twin, colNormSq, yPredLinear, K and yPredQuad of the components the model holds, the residual;
// *loss_old = ||residual||^2 / n
int hazan_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const CfmView& M, const HazanCfg& cfg, HazanState* S,
                    double* loss_old);
// hazan.nim:140-202 with `it` = self.it: one outer iteration from the start vector (host, d doubles, not normalised);
// *n_components is the model's count before and after
int hazan_iter(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const HazanCfg& cfg, HazanState* S, int64_t it, const double* start,
               int32_t* n_components, double* record);

}  // namespace nfm
