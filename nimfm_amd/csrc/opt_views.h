// nimfm_amd/csrc/opt_views.h -- optimizer parameter/state views passed by value to kernels.
#pragma once
#include "common.h"
#include "seq_route.h"

namespace nfm {

// OPT_PSGD: the reference's mini-batch proximal SGD (optimizer/minibatch_psgd.nim)
// OPT_CD: coordinate descent (optimizer/cd.nim), a whole-dataset iteration per nfm_opt_epoch call (cd.h)
// OPT_PGD: the full-batch proximal gradient solvers (optimizer/pgd.nim, fista.nim, nmapgd.nim), one iteration per nfm_opt_epoch call (pgd.h)
// OPT_KATYUSHA: the variance-reduced accelerated solver (optimizer/katyusha.nim), one outer iteration per nfm_opt_epoch call (katyusha.h)
// OPT_HAZAN: Hazan's algorithm for the convex model (optimizer/hazan.nim), one outer iteration per nfm_hazan_iter call (cfm.h)
// OPT_GCD: greedy coordinate descent for the convex model (optimizer/greedy_cd.nim), stepped by nfm_gcd_outer_begin / nfm_gcd_inner / nfm_gcd_outer_end (gcd.h)
// OPT_PSGD_SEQ: the reference's PSGD (optimizer/psgd.nim), one sample at a time with the lazily caught-up L1 / L21 regularisers (psgd_seq.h)
enum { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_PSGD = 2, OPT_CD = 3, OPT_PGD = 4, OPT_KATYUSHA = 5, OPT_HAZAN = 6, OPT_GCD = 7, OPT_PSGD_SEQ = 8 };

struct OptView {
  // hyper-parameters (newSGD optimizer/sgd.nim:23-52, newAdaGrad optimizer/adagrad.nim:20-44)
  double eta0, alpha0, alpha, beta, power, eps, loss_param;
  // SGD mini-batch rule: at most this many of a batch's per-sample steps on one coordinate are SUMMED (the reference's
  // Hogwild threads apply theirs at full strength too, optimizer/sgd_multi.nim:83-101); a coordinate touched c > cap
  // times receives cap / c of the sum.  1 (default): the per-coordinate mean
  double touch_cap;
  // AdaGrad mini-batch rule (round 5): g_norm of a coordinate grows by the batch's  sum g^2 + ada_cross ((sum g)^2 - sum g^2)  -- the
  // cross products of the samples' gradients, all taken from the batch-start parameters: the norm sees how far the batch AGREES on a
  // coordinate (what NFM_DP_STATE_CROSS does for the ranks of a data-parallel group, dp.h).  0 (default): the samples' squares alone
  double ada_cross;
  int32_t loss, sched, track_viol, pad_;
  // AdaGrad state, device layout: G/N [nb][da][Kp] (padding: G = 0, N = eps), Gw/Nw [d],
  // gsc[0] = g_sum.intercept, gsc[1] = g_norm.intercept
  double* G;
  double* N;
  double* Gw;
  double* Nw;
  double* gsc;
  // MBPSGD (newMBPSGD, optimizer/minibatch_psgd.nim:24-65): gamma, miniBatchSize as a double, NFM_REG_*
  double gamma, bsize;
  int32_t reg, reg_transpose;
  // pgd.predictAllWithGrad (optimizer/pgd.nim:70-103): when set, the column phase of OPT_PSGD stores the batch
  // gradient here (device layout of P, [d], one scalar) instead of stepping the parameters
  double* gradP;
  double* gradw;
  double* gradb;
};

// ---- NFM_MODE_SEQUENTIAL: what seq_route.h decides by ----
static_assert(SEQ_KIND_FM == NFM_KIND_FM && SEQ_KIND_FFM == NFM_KIND_FFM, "seq_route.h restates these two");
inline SeqShape seq_shape(const ModelView& M, int m_cap, int64_t ns, int64_t nnz, bool ada, int n_cu) {
  return {M.kind, M.degree, M.nb, M.kc, M.k, M.Kp, M.n_aug, M.fit_intercept, M.d, M.da, M.bs, M.rs, m_cap, ns, nnz, ada, n_cu};
}
// ---- seq.hip: one workgroup, one sample in flight; M as seq_row_view gives it, the kernel by seq_one_wg_route ----
int launch_sequential(nfm_ctx* ctx, int opt_kind, const CsrView& X, const ModelView& M, const OptView& O,
                      const int64_t* perm_dev, int64_t begin, int64_t end, int64_t it0, int m_cap,
                      double* out2_dev /*{loss_sum, viol_sum}*/, const SeqKnobs& K);
// ---- seqwin.hip: the same order as launch_sequential, run as a dependency window over the chip ----
struct SeqWin {           // kept on the optimizer between calls
  DevBuf prev;            // [nnz] per stored entry: previous position of the call with the same feature
  DevBuf prevq, next;     // [nnz] that feature's entry index in the previous sample's row; next position with the feature
  DevBuf scales, mail, ctl, fw, trace;
  DevBuf snap;            // the model's arena (+ AdaGrad: the state arena) as it was when the call began (abort: put back)
  int64_t fallbacks = 0;  // calls that ended in the one-workgroup kernel after an abort (forgotten one at a time: 16 clean calls each)
  int64_t clean_calls = 0;
  bool valid = false, had_perm = false;
  uint64_t ds_uid = 0;
  int64_t begin = 0, end = 0, nnz = 0;
};
// the model as the window kernels see it: where the route says so (WinRoute::two_block), a 65 ... 128-factor FM read as two
// blocks of 64
inline ModelView seq_window_view(const ModelView& M, const WinRoute& R) {
  if (!R.two_block) return M;
  ModelView V = M;
  V.nb = R.nb;
  V.kc = V.nb;
  V.Kp = R.Kp;
  V.L = kWave / 2;
  V.k = kWave;
  V.bs = 1;
  V.rs = V.nb;
  return V;
}
// the model as the one-sample-in-flight kernel sees it: a wide FM of one order whose kc blocks lie feature-major is ONE row of
// kc * Kp factors per feature (padding zeros inside the row add nothing to the ascending factor sum, sgd.nim:172-173)
inline ModelView seq_row_view(const ModelView& M) {
  if (!(M.kind == NFM_KIND_FM && M.kc > 1 && M.nb == M.kc && M.bs == 1 && M.rs == M.nb)) return M;
  ModelView V = M;
  V.Kp = M.nb * M.Kp;
  V.k = V.Kp;
  V.L = 64;
  V.nb = 1;
  V.kc = 1;
  V.bs = M.da;
  V.rs = 1;
  return V;
}
// launch_sequential_window's third outcome besides NFM_OK and an error: the window could not run to its end (the route does not
// fit the device, the kernel does not fit a CU, or a wait inside it timed out and the launch aborted).  Parameters and state of the call may be partly
// updated: the caller puts its snapshot back and runs launch_sequential over the same range.
constexpr int NFM_WIN_FALLBACK = 1;
int launch_sequential_window(nfm_ctx* ctx, int opt_kind, const CsrView& X, const ModelView& M, const OptView& O,
                             const int64_t* perm_dev, int64_t begin, int64_t end, int64_t it0, const WinRoute& R, const SeqKnobs& K,
                             double* out2_dev /*{loss_sum, viol_sum}*/, SeqWin* sw, uint64_t ds_uid, bool perm_is_callers);
// AdaGrad finalize (optimizer/adagrad.nim:65-84): all parameters from the state with it' = it-1
int launch_adagrad_finalize(nfm_ctx* ctx, const ModelView& M, const OptView& O, int64_t it);

}  // namespace nfm
