// nimfm_amd/csrc/katyusha.hip -- Katyusha (optimizer/katyusha.nim:76-269) with params, z, y, tilde, next_tilde, grads_ave and
// the mini-batch gradients resident on the device.
//
// One inner iteration (katyusha.nim:99-137) is
//   the mini-batch gradient at params and at tilde_params: the OPT_PSGD row / column phase in its gradient mode, once per
//     parameter set, over ONE mini-batch of the epoch's plan (the sums per coordinate in the stream's sample order),
//   k_kat_mark: the features that mini-batch touches get the iteration's stamp,
//   k_kat_dense: ONE pass over all parameters -- grads = grads_ave + (g(params) - g(tilde)) on stamped rows, the z step and
//     shrink, the row-local prox, the y update, the next_tilde accumulation and the NEXT iteration's params.  For the
//     column-coupled operators the pass splits at the prox (step | launch_prox_coupled | the rest).
// The end of the epoch (k_kat_end) scales next_tilde, sums computeViol in a fixed order, moves tilde and writes finalize's
// model into the model handle's arena.  No floating-point atomics: two runs give the same bits.
//
// The reference's quirks, kept:
//   * Params.add steps w only when fitLinear and the intercept only when fitIntercept AND fitLinear (params.nim:41-48); scale
//     gates on the flags; `<-` copies everything.  With fitIntercept and not fitLinear the intercept only decays, and
//     next_tilde's intercept stays 0.  next_tilde is created zero and cleared under the flags (katyusha.nim:93-97), so
//     without fitLinear (fitIntercept) tilde's w (intercept) is 0 from the first epoch on.
//   * fit calls finalize(sfm, tilde, y, float(maxIterInner), tau1, tau2) on a proc declared (..., tau1, tau2, m)
//     (katyusha.nim:56-57, 238, 269): the model is (tau1 tau2 tilde + (1 - m - tau1) y) / (tau1 tau2 + 1 - m - tau1), formed as
//     finalize forms it (:59-73): the product, `+=`, then the element-wise division of tensor.nim:453-455.
//   * lossVal is the loss at the snapshot the epoch STARTED from (the yPred of the last predictAllWithGrad, :241-244).
//   * nothing is carried between fits.
#include <math.h>

#include <algorithm>

#include "fm_device.h"
#include "katyusha.h"
#include "prox_dev.h"

namespace nfm {

enum { KAT_ALL = 0, KAT_STEP = 1, KAT_REST = 2 };

struct KatSetPtr {
  double *P, *w, *sc;
};

struct KatArgs {
  ModelView M;  // geometry and flags
  KatSetPtr x, z, y, nx;           // params, z_params, y_params, next_tilde_params
  KatSetPtr tl, ga, gx, gt;        // tilde_params, grads_ave, the mini-batch gradient at params / at tilde_params (read only)
  const int32_t* stamp;            // [da]
  int32_t cur;
  double eta, invP, invW, invB, lam, tau1, tau2, tau3, thP, thW, thB;  // th*: theta_pow_* of this inner iteration
  int32_t reg, reg_transpose, phase;
  double* norms;  // [nb][da] (SquaredL21)
};

// The features of one mini-batch of the plan (ucol[u0 .. u1)) get the inner iteration's stamp.
__global__ __launch_bounds__(kBlock) void k_kat_mark(const int32_t* __restrict__ ucol, int64_t u0, int64_t u1, int64_t da, int32_t* stamp,
                                                     int32_t cur) {
  const int64_t u = u0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u >= u1) return;
  const int64_t j = ucol[u];
  if (j >= 0 && j < da) stamp[j] = cur;
}

// katyusha.nim:105-137 after the mini-batch gradients, and :101-102 of the NEXT inner iteration, per element in the
// reference's order of operations.  grid (G, nb + 1): y < nb walks device block y, y == nb the linear term and the intercept.
template <int L>
__global__ __launch_bounds__(kBlock) void k_kat_dense(KatArgs a) {
  constexpr int R = kWave / L;
  const ModelView& M = a.M;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int g = lane / L, l = lane % L, b = blockIdx.y;
  const double lam = a.lam;
  if (b < M.nb) {
    const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * R;
    for (int64_t j0 = ((int64_t)blockIdx.x * kWavesPerBlock + wv) * R; j0 < M.da; j0 += stride) {  // uniform per wavefront
      const int64_t j = j0 + g;
      const bool act = j < M.da;  // inactive lanes keep taking part in the shuffles
      const size_t e = M.row(b, act ? j : 0) * M.Kp + 2 * l;
      double2 p = {0.0, 0.0};
      if (a.phase != KAT_REST) {
        double2 zo = {0.0, 0.0}, gr = {0.0, 0.0};
        if (act) {
          zo = *reinterpret_cast<const double2*>(a.z.P + e);
          gr = *reinterpret_cast<const double2*>(a.ga.P + e);
          if (a.stamp[j] == a.cur) {  // grads = grads_ave + delta: delta is nonzero on the mini-batch's features only
            const double2 u = *reinterpret_cast<const double2*>(a.gx.P + e), v = *reinterpret_cast<const double2*>(a.gt.P + e);
            gr.x += u.x - v.x;
            gr.y += u.y - v.y;
          }
        }
        p.x = (zo.x + -a.eta * gr.x) * a.invP;  // Params.step (params.nim:90-98)
        p.y = (zo.y + -a.eta * gr.y) * a.invP;
        NFM_ROW_LOCAL_PROX(L, a.reg, a.reg_transpose, lam, p, act, l, a.norms[(size_t)b * M.da + j]);
        if (act) *reinterpret_cast<double2*>(a.z.P + e) = p;
      } else if (act) {
        p = *reinterpret_cast<const double2*>(a.z.P + e);
      }
      if (a.phase == KAT_STEP || !act) continue;  // (uniform per wavefront but for the tail, which has no shuffles left)
      const double2 t = *reinterpret_cast<const double2*>(a.tl.P + e);
      double2 yv = *reinterpret_cast<const double2*>(a.y.P + e), nv = *reinterpret_cast<const double2*>(a.nx.P + e), xv;
      yv.x *= a.tau3;  // :130-132
      yv.y *= a.tau3;
      yv.x += a.tau2 * t.x;
      yv.y += a.tau2 * t.y;
      yv.x += a.tau1 * p.x;
      yv.y += a.tau1 * p.y;
      nv.x += a.thP * yv.x;  // :133
      nv.y += a.thP * yv.y;
      xv.x = p.x * a.tau1;  // nmapgd.extrapolate (nmapgd.nim:133-138) of the next inner iteration
      xv.y = p.y * a.tau1;
      xv.x += a.tau2 * t.x;
      xv.y += a.tau2 * t.y;
      xv.x += a.tau3 * yv.x;
      xv.y += a.tau3 * yv.y;
      *reinterpret_cast<double2*>(a.y.P + e) = yv;
      *reinterpret_cast<double2*>(a.nx.P + e) = nv;
      *reinterpret_cast<double2*>(a.x.P + e) = xv;
    }
  } else if (a.phase != KAT_REST) {  // the linear term and the intercept ride with the step
    if (M.fit_linear)  // without fitLinear no set's w ever moves (params.nim:41-45,63-64)
      for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < M.d; j += (int64_t)gridDim.x * kBlock) {
        double gw = a.ga.w[j];
        if (a.stamp[j] == a.cur) gw += a.gx.w[j] - a.gt.w[j];
        const double zw = (a.z.w[j] + -a.eta * gw) * a.invW, tw = a.tl.w[j];
        double yw = a.y.w[j] * a.tau3;
        yw += a.tau2 * tw;
        yw += a.tau1 * zw;
        double xw = zw * a.tau1;
        xw += a.tau2 * tw;
        xw += a.tau3 * yw;
        a.z.w[j] = zw;
        a.y.w[j] = yw;
        a.nx.w[j] += a.thW * yw;
        a.x.w[j] = xw;
      }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const bool fi = M.fit_intercept, both = M.fit_intercept && M.fit_linear;
      double gb = a.ga.sc[SC_INTERCEPT];
      if (fi) gb += a.gx.sc[SC_INTERCEPT] - a.gt.sc[SC_INTERCEPT];  // minibatch_psgd.nim:87-88
      double zb = a.z.sc[SC_INTERCEPT], yb = a.y.sc[SC_INTERCEPT];
      const double tb = a.tl.sc[SC_INTERCEPT];
      if (both) zb += -a.eta * gb;  // params.nim:47 gates the step on grad.fitLinear
      if (fi) zb *= a.invB;
      if (fi) yb *= a.tau3;
      if (both) {
        yb += a.tau2 * tb;
        yb += a.tau1 * zb;
        a.nx.sc[SC_INTERCEPT] += a.thB * yb;
      }
      double xb = zb;  // `<-` copies, `*=` gates on fitIntercept, add on both flags
      if (fi) xb *= a.tau1;
      if (both) {
        xb += a.tau2 * tb;
        xb += a.tau3 * yb;
      }
      a.z.sc[SC_INTERCEPT] = zb;
      a.y.sc[SC_INTERCEPT] = yb;
      a.x.sc[SC_INTERCEPT] = xb;
    }
  }
}

// katyusha.nim:153 (next_tilde.scale), :235 (computeViol(next_tilde, tilde)), :236 (tilde <- next_tilde) and finalize (:59-73)
// with the arguments as fit passes them (:238, :269), into the model handle's arena.  grid (G, 2): y == 0 the flat P arena
// (padding is zero in every set and stays zero: den != 0), y == 1 the linear term and the intercept.
struct KatEndArgs {
  KatSetPtr nx, tl, y, model;
  int64_t nP, d;
  int32_t fit_linear, fit_intercept, G;
  double coefP, coefW, coefB;  // (1 - theta) / (1 - theta_pow)
  double c1, c2, den;          // finalize's m * tau2, 1 - tau1 - tau2 and tau2 * m + 1 - tau1 - tau2 under its own names
  double* partial;             // [2][G][4]
  double* rec;
};
__global__ __launch_bounds__(kBlock) void k_kat_end(KatEndArgs a) {
  __shared__ double red[kBlock];
  double viol = 0.0;
  if (blockIdx.y == 0) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < a.nP; e += (int64_t)gridDim.x * kBlock) {
      const double nv = a.nx.P[e] * a.coefP, dv = nv - a.tl.P[e];
      viol += dv * dv;
      a.tl.P[e] = nv;
      double v = a.c1 * nv;
      v += a.c2 * a.y.P[e];
      a.model.P[e] = v / a.den;
    }
  } else {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.d; j += (int64_t)gridDim.x * kBlock) {
      const double nv = a.fit_linear ? a.nx.w[j] * a.coefW : a.nx.w[j], dv = nv - a.tl.w[j];
      if (a.fit_linear) viol += dv * dv;
      a.tl.w[j] = nv;
      if (a.fit_linear) {
        double v = a.c1 * nv;
        v += a.c2 * a.y.w[j];
        a.model.w[j] = v / a.den;
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const double nv = a.fit_intercept ? a.nx.sc[SC_INTERCEPT] * a.coefB : a.nx.sc[SC_INTERCEPT], dv = nv - a.tl.sc[SC_INTERCEPT];
      a.rec[RS_VIOLB] = a.fit_intercept ? dv * dv : 0.0;
      a.tl.sc[SC_INTERCEPT] = nv;
      if (a.fit_intercept) {
        double v = a.c1 * nv;
        v += a.c2 * a.y.sc[SC_INTERCEPT];
        a.model.sc[SC_INTERCEPT] = v / a.den;
      }
    }
  }
  red[threadIdx.x] = viol;
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {  // one fixed tree
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x < 4) a.partial[((size_t)blockIdx.y * a.G + blockIdx.x) * 4 + threadIdx.x] = threadIdx.x == 0 ? red[0] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- host
KatState::~KatState() {
  if (pin) (void)hipHostFree(pin);
}

namespace {

constexpr int kKatPin = 2 + RS_PART + 8;  // {loss_sum, viol of a gradient pass}, then the end-of-epoch record

KatSetPtr ptr(const PgdSet& s) { return KatSetPtr{s.P(), s.w(), s.sc()}; }
PgdRef ref(const PgdSet& s) { return PgdRef{s.P(), s.w(), s.sc()}; }
ModelView view(const ModelView& M, const PgdSet& s) {
  ModelView V = M;
  V.P = s.P();
  V.w = s.w();
  V.sc = s.sc();
  return V;
}
bool coupled(const KatCfg& c) { return (c.reg == NFM_REG_SQUAREDL12 && c.reg_transpose) || c.reg == NFM_REG_SQUAREDL21; }

int copy_set(nfm_ctx* ctx, const PgdSet& dst, const double* P, const double* w, const double* sc, const ModelView& M) {  // Params.`<-`
  const int64_t nPd = (int64_t)M.nb * M.da * M.Kp;
  if (nPd > 0) NFM_HIP_CHECK(hipMemcpyAsync(dst.P(), P, sizeof(double) * nPd, hipMemcpyDeviceToDevice, ctx->stream));
  if (M.d > 0) NFM_HIP_CHECK(hipMemcpyAsync(dst.w(), w, sizeof(double) * M.d, hipMemcpyDeviceToDevice, ctx->stream));
  NFM_HIP_CHECK(hipMemcpyAsync(dst.sc(), sc, sizeof(double) * SC_COUNT, hipMemcpyDeviceToDevice, ctx->stream));
  return NFM_OK;
}

OptView grad_view(const KatCfg& c) {
  OptView O{};
  O.loss = c.loss;
  O.loss_param = c.loss_param;
  O.touch_cap = 1.0;
  O.eta0 = 1.0;
  O.reg = c.reg;
  O.reg_transpose = c.reg_transpose;
  return O;
}

// predictAllWithGrad(tilde) -> grads_ave and the loss sum of that snapshot (katyusha.nim:216-217, 261-262)
int snapshot_gradient(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const ModelView& M, KatState* S) {
  TimedLaunch tl(ctx, "kat_full_grad");
  NFM_HIP_CHECK(hipMemsetAsync(S->gave.buf.p, 0, S->gave.buf.bytes, ctx->stream));
  double out2[2] = {0.0, 0.0};
  S->Wg.batch_begin = 0;
  S->Wg.batch_end = -1;
  NFM_TRY(full_gradient(ctx, X, uid, view(M, S->tilde), grad_view(S->cfg), S->gplan, S->Wg, S->gave.P(), S->gave.w(), S->gave.sc() + SC_INTERCEPT, 0, out2));
  S->loss_sum = out2[0];
  S->grad_stale = false;
  return NFM_OK;
}

// updateGradient (minibatch_psgd.nim:67-88) of mini-batch b of the epoch's plan at one parameter set: coef = dloss / miniBatchSize,
// summed per coordinate in the stream's sample order.  Rows of features the mini-batch does not touch keep what they held.
int batch_gradient(nfm_ctx* ctx, const CsrView& X, const ModelView& M, KatState* S, const PgdSet& at, const PgdSet& g, int64_t b) {
  OptView O = grad_view(S->cfg);
  O.bsize = (double)S->cfg.batch;
  O.gradP = g.P();
  O.gradw = g.w();
  O.gradb = g.sc() + SC_INTERCEPT;
  S->W.use_graph = false;
  S->W.batch_begin = b;
  S->W.batch_end = b + 1;
  return mb_fm_epoch(ctx, OPT_PSGD, X, view(M, at), O, *S->plan, S->W, 0, S->pin, 0, /*defer_sync=*/true);
}

}  // namespace

int kat_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, KatState* S) {
  const KatCfg& c = S->cfg;
  NFM_CHECK(X.n > 0, NFM_ERR_INVALID, "the dataset has no samples");
  S->fit_ready = false;
  S->n = X.n;
  S->m_inner = (X.n - 1) / c.batch + 1;  // katyusha.nim:207
  NFM_CHECK(S->m_inner <= (int64_t)2147483647 / c.batch, NFM_ERR_INVALID,
            "miniBatchSize %lld: one epoch's index stream (%lld mini-batches) does not fit a plan of 2^31-1 positions", (long long)c.batch,
            (long long)S->m_inner);
  S->tau2 = c.tau2 < 0 ? 1.0 / (2.0 * (double)c.batch) : c.tau2;  // :208-213
  S->tau1 = c.tau1 < 0 ? S->tau2 : c.tau1;
  {
    const double m = (double)S->m_inner, den = S->tau1 * S->tau2 + 1.0 - m - S->tau1;
    NFM_CHECK(den != 0.0 && den == den, NFM_ERR_INVALID,
              "tau1 = %g, tau2 = %g with %lld inner iterations make finalize's divisor tau1 tau2 + 1 - m - tau1 zero", S->tau1, S->tau2,
              (long long)S->m_inner);
  }
  PgdSet* sets[] = {&S->x, &S->z, &S->y, &S->tilde, &S->next, &S->gave, &S->gx, &S->gt};
  for (PgdSet* s : sets) NFM_TRY(pgd_alloc_set(ctx, M, *s, true));
  NFM_TRY(S->stamp.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(M.da, 1)));
  NFM_HIP_CHECK(hipMemsetAsync(S->stamp.p, 0, S->stamp.bytes, ctx->stream));
  S->stamp_cur = 0;
  NFM_TRY(S->prox.ensure(sizeof(double) * prox_scratch_doubles(M)));
  NFM_TRY(S->partial.ensure(sizeof(double) * 4 * 2 * (size_t)kPgdMaxBlocks));
  NFM_TRY(S->rec.ensure(sizeof(double) * (RS_PART + 8)));
  NFM_HIP_CHECK(hipMemsetAsync(S->rec.p, 0, S->rec.bytes, ctx->stream));
  if (!S->pin) NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&S->pin), sizeof(double) * kKatPin));
  // y, z, tilde <- params (:188-193); params itself is formed by the first extrapolation of every epoch
  NFM_TRY(copy_set(ctx, S->y, M.P, M.w, M.sc, M));
  NFM_TRY(copy_set(ctx, S->z, M.P, M.w, M.sc, M));
  NFM_TRY(copy_set(ctx, S->tilde, M.P, M.w, M.sc, M));
  NFM_TRY(snapshot_gradient(ctx, X, uid, M, S));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  S->fit_uid = uid;
  S->fit_serial = serial;
  S->fit_ready = true;
  return NFM_OK;
}

int kat_epoch(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const ModelView& M, KatState* S, const int64_t* perm, int64_t begin,
              int64_t end, double* loss_sum, double* viol_sum) {
  const KatCfg& c = S->cfg;
  hipStream_t st = ctx->stream;
  const int64_t B = c.batch, m = S->m_inner, ns = end - begin;
  const double tau1 = S->tau1, tau2 = S->tau2, tau3 = 1 - tau1 - tau2;
  // the full gradient at the snapshot the previous epoch left (:261-262): a fit that converged or ended pays for none
  if (S->grad_stale) NFM_TRY(snapshot_gradient(ctx, X, uid, M, S));
  const double epoch_loss = S->loss_sum;
  // the plan of the epoch's index stream, uploaded once
  if (!perm) {
    S->ident.resize((size_t)ns);
    for (int64_t p = 0; p < ns; ++p) S->ident[(size_t)p] = (begin + p) % X.n;
    perm = S->ident.data() - begin;
  }
  {
    TimedLaunch tl(ctx, "plan_build");
    if (!S->plan) S->plan.reset(new Plan());
    const bool sort_by_count = M.Kp * (int)sizeof(double) >= 128;
    NFM_TRY(plan_build(ctx, X, M.n_aug, perm, begin, end, B, false, false, false, sort_by_count, S->plan.get()));
  }
  const Plan& PL = *S->plan;
  NFM_CHECK(PL.n_batches == m, NFM_ERR_INVALID, "the plan holds %lld mini-batches, not %lld", (long long)PL.n_batches, (long long)m);
  // :84-97
  const double md = (double)m;
  const double thP = 1.0 + std::min(c.eta * c.beta, 1.0 / (4.0 * md)), thW = 1.0 + std::min(c.eta * c.alpha, 1.0 / (4.0 * md)),
               thB = 1.0 + std::min(c.eta * c.alpha0, 1.0 / (4.0 * md));
  double powP = 1.0, powW = 1.0, powB = 1.0;
  NFM_HIP_CHECK(hipMemsetAsync(S->next.buf.p, 0, S->next.buf.bytes, st));
  // :101-102 of the first inner iteration; the dense pass leaves every later one's
  NFM_TRY(launch_pgd_mix(ctx, M, ref(S->x), ref(S->z), ref(S->tilde), ref(S->y), true, tau1, tau2, tau3));
  KatArgs a{};
  a.M = M;
  a.x = ptr(S->x); a.z = ptr(S->z); a.y = ptr(S->y); a.nx = ptr(S->next);
  a.tl = ptr(S->tilde); a.ga = ptr(S->gave); a.gx = ptr(S->gx); a.gt = ptr(S->gt);
  a.stamp = S->stamp.as<int32_t>();
  a.eta = c.eta;
  a.invP = 1.0 / (1.0 + c.eta * c.beta);
  a.invW = 1.0 / (1.0 + c.eta * c.alpha);
  a.invB = 1.0 / (1.0 + c.eta * c.alpha0);
  a.lam = c.gamma * c.eta / (1.0 + c.beta * c.eta);  // :124
  a.tau1 = tau1; a.tau2 = tau2; a.tau3 = tau3;
  a.reg = c.reg; a.reg_transpose = c.reg_transpose;
  a.norms = S->prox.as<double>();
  const int R = kWave / M.L;
  const int G = (int)std::min<int64_t>(kPgdMaxBlocks, std::max<int64_t>((std::max<int64_t>(M.da, M.d) + kWavesPerBlock * R - 1) / (kWavesPerBlock * R), 1));
  auto dense = [&](int phase) {
    a.phase = phase;
    with_lanes(M.L, [&](auto L) { hipLaunchKernelGGL((k_kat_dense<L()>), dim3((unsigned)G, (unsigned)(M.nb + 1)), dim3(kBlock), 0, st, a); });
  };
  const ModelView Mz = view(M, S->z);
  for (int64_t b = 0; b < m; ++b) {
    NFM_TRY(batch_gradient(ctx, X, M, S, S->x, S->gx, b));
    NFM_TRY(batch_gradient(ctx, X, M, S, S->tilde, S->gt, b));
    TimedLaunch tl(ctx, "kat_dense");
    if (S->stamp_cur == 2147483647) {  // (2^31 inner iterations of one fit: the stamps start over)
      NFM_HIP_CHECK(hipMemsetAsync(S->stamp.p, 0, S->stamp.bytes, st));
      S->stamp_cur = 0;
    }
    a.cur = ++S->stamp_cur;
    const int64_t u0 = PL.bat_uoff[b], u1 = PL.bat_uoff[b + 1];
    if (u1 > u0)
      hipLaunchKernelGGL(k_kat_mark, dim3((unsigned)((u1 - u0 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, PL.ucol.as<int32_t>(), u0, u1, M.da,
                         S->stamp.as<int32_t>(), a.cur);
    a.thP = powP; a.thW = powW; a.thB = powB;
    if (coupled(c)) {  // the pass splits at the prox
      dense(KAT_STEP);
      launch_prox_coupled(ctx, Mz, c.reg, a.lam, S->prox.as<double>());
      dense(KAT_REST);
    } else {
      dense(KAT_ALL);
    }
    NFM_HIP_CHECK(hipGetLastError());
    powP *= thP;  // :135-137
    powW *= thW;
    powB *= thB;
  }
  {
    TimedLaunch tl(ctx, "kat_end");
    KatEndArgs q{};
    q.nx = ptr(S->next); q.tl = ptr(S->tilde); q.y = ptr(S->y); q.model = KatSetPtr{M.P, M.w, M.sc};
    q.nP = (int64_t)M.nb * M.da * M.Kp;
    q.d = M.d;
    q.fit_linear = M.fit_linear; q.fit_intercept = M.fit_intercept;
    q.G = (int)std::min<int64_t>(kPgdMaxBlocks, std::max<int64_t>((std::max<int64_t>(q.nP, M.d) + kBlock - 1) / kBlock, 1));
    q.coefP = (1.0 - thP) / (1.0 - powP);  // :150-152
    q.coefW = (1.0 - thW) / (1.0 - powW);
    q.coefB = (1.0 - thB) / (1.0 - powB);
    // finalize(sfm, tilde, y, float(maxIterInner), tau1, tau2) read through its own parameter names (tau1, tau2, m)
    const double f_tau1 = md, f_tau2 = tau1, f_m = tau2;
    q.c1 = f_m * f_tau2;
    q.c2 = 1 - f_tau1 - f_tau2;
    q.den = f_tau2 * f_m + 1.0 - f_tau1 - f_tau2;
    q.partial = S->partial.as<double>();
    q.rec = S->rec.as<double>();
    hipLaunchKernelGGL(k_kat_end, dim3((unsigned)q.G, 2), dim3(kBlock), 0, st, q);
    NFM_TRY(launch_pgd_finish(ctx, q.partial, 2, q.G, q.rec));
    NFM_HIP_CHECK(hipMemcpyAsync(S->pin + 2, S->rec.p, sizeof(double) * (RS_PART + 8), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  S->grad_stale = true;
  const double* r = S->pin + 2;
  double viol = r[RS_PART + 0];  // computeViol (utils.nim:5-17): P, then w, then the intercept
  viol += r[RS_PART + 4];
  viol += r[RS_VIOLB];
  if (loss_sum) *loss_sum = epoch_loss;
  if (viol_sum) *viol_sum = viol;
  return NFM_OK;
}

}  // namespace nfm
