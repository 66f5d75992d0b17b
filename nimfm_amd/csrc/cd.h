// nimfm_amd/csrc/cd.h -- coordinate descent (optimizer/cd.nim, fit_linear.nim:5-37) on the device: the level schedule and
// the per-optimizer state of cd.hip.
#pragma once
#include "common.h"

namespace nfm {

// the ANOVA degree CD takes (the derivative dA[0 .. degree) of cd.nim:30-34 is kept in registers)
constexpr int kCdMaxDeg = 10;

// the regulariser of plain CD (no proximal step); newPCD takes NFM_REG_L1, NFM_REG_SQUAREDL12 or NFM_REG_OMEGATI
constexpr int32_t kCdNoReg = -1;

// hyper-parameters of one fit, scaled as cd.nim:117-127 scales them (alpha0 * n, alpha * n, beta * n; pcd.nim:137 gamma * n)
struct CdParams {
  double alpha0, alpha, beta;  // as the caller gave them (newCD, cd.nim:12-13; newPCD, pcd.nim:17-20)
  int32_t loss;
  double loss_param;
  double gamma = 0.0;          // newPCD's sparsity strength
  int32_t reg = kCdNoReg;      // kCdNoReg: plain CD
  int32_t reg_transpose = 0;   // SquaredL12's transpose (squaredl12.nim:85-88)
  bool block = false;          // newPBCD (pbcd.nim): the P sweeps step a feature's whole row; reg is L1, L21, SquaredL21 or
                               // OmegaCS
  // SquaredL12 column-wise and OmegaTI (PCD), SquaredL21 and OmegaCS (PBCD): a feature's prox reads a running value over every earlier
  // feature (run schedule)
  bool chained() const {
    return reg == NFM_REG_OMEGATI || (reg == NFM_REG_SQUAREDL12 && reg_transpose) ||
           (block && (reg == NFM_REG_SQUAREDL21 || reg == NFM_REG_OMEGACS));
  }
};

struct CdState {
  // ---- the schedule: built once per dataset (uid) ----
  uint64_t sched_uid = 0;
  bool sched_ready = false;
  int64_t n = 0, d = 0, nnz = 0;
  DevBuf rptr, ridx, rval;  // the rows with their column ids ascending (int64[n+1], int32[nnz], f64[nnz])
  DevBuf cptr, crow, cval;  // the column twin, sample ids ascending inside a column
  DevBuf order;             // int32[d]: the features sorted by (level, j)
  DevBuf goff;              // int64[G+1]: offsets of the non-empty levels in `order`
  std::vector<int64_t> goff_h;
  int64_t widest = 0;
  // the run schedule of the chained regularisers (pcd.hip): runs of consecutive features j, pairwise sample-disjoint
  DevBuf roff;  // int64[R+1]: the first feature of every run
  std::vector<int64_t> roff_h;
  int64_t widest_run = 0;
  // ---- one fit (nfm_cd_begin_fit) ----
  uint64_t fit_uid = 0, fit_serial = 0;
  bool fit_ready = false;
  double a0n = 0, an = 0, bn = 0, mu = 1;  // alpha0 * n, alpha * n, beta * n, loss.mu
  DevBuf yp, cache, A, colsq, out;         // out: |update| per coordinate in the reference's order, then the loss sum
  double gn = 0;                           // PCD: gamma * n
  DevBuf rcache;                           // PCD SquaredL12 row-wise: cache[j] (squaredl12.nim:166-172)
  DevBuf sgrad;                            // PCD run schedule: (update, invStepSize, psj, delta) per feature, [4][d + nAug]
  DevBuf chain;                            // PCD run schedule: the regulariser's running state of the current component
  // PBCD (pbcd.hip): anova's table A [degree + 1][n][k] and its derivative dA [degree][n][k] for every component at once;
  // per feature the row scratch (gradient, then the pre-prox row) and delta, [d + nAug][k] each; per feature invStepSize,
  // the pre-prox row's norm, the chain's scale and norms[j] ([4][d + nAug]); chain[0] is SquaredL21's running cache, chain
  // as a whole OmegaCS's cache and dcache
  DevBuf bA, bdA, brow, bdelta, bfeat;
  int64_t n_out = 0;
  double* out_h = nullptr;  // pinned copy of `out`
  void* graph_exec = nullptr;
  uint64_t graph_uid = 0, graph_serial = 0;
  void drop_graph();
  ~CdState();
};

// the schedule of the dataset (copies its arrays back once per dataset); n_levels / widest of the P sweep, augments included
// (runs instead of levels when `runs`: the chained regularisers of PCD)
int cd_schedule(nfm_ctx* ctx, const CsrView& X, uint64_t uid, int n_aug, CdState* S, int64_t* n_levels, int64_t* widest,
                bool runs = false);
// cd.nim:128-153: the schedule, colNormSq, yPred from the model's current parameters (unit scales)
int cd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, int n_components,
                 const CdParams& P, CdState* S);
// one iteration of cd.nim:156-175; loss_sum = sum_i loss(y_i, yPred_i) after it, viol_sum as the reference sums it
int cd_epoch(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int n_components, const CdParams& P, CdState* S,
             double* loss_sum, double* viol_sum);


// ---- pbcd.hip: newPBCD's part of the fit and of the iteration (cd_begin_fit and cd_epoch call them when P.block) ----
struct CdDev;
// pbcd.nim:252-271: yPred = linear + intercept, then per order precomputeAnova and yPred += A[degree - order]
int pbcd_begin_fit(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int n_components, const CdParams& P, CdState* S, const CdDev& D);
// pbcd.nim:292-299: the epochs of every order, after CD's intercept and w sweep and before the loss sum
int pbcd_issue_orders(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int n_components, const CdParams& P, CdState* S, const CdDev& D);

}  // namespace nfm
