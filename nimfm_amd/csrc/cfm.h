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
// hazan.nim:59-134: the twin, colNormSq, yPredLinear, K and yPredQuad of the components the model holds, the residual;
// *loss_old = ||residual||^2 / n
int hazan_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const CfmView& M, const HazanCfg& cfg, HazanState* S,
                    double* loss_old);
// hazan.nim:140-202 with `it` = self.it: one outer iteration from the start vector (host, d doubles, not normalised);
// *n_components is the model's count before and after
int hazan_iter(nfm_ctx* ctx, const CsrView& X, const CfmView& M, const HazanCfg& cfg, HazanState* S, int64_t it, const double* start,
               int32_t* n_components, double* record);

}  // namespace nfm
