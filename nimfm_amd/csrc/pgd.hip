// nimfm_amd/csrc/pgd.hip -- PGD, FISTA and NMAPGD (optimizer/pgd.nim:106-217, fista.nim:46-141, nmapgd.nim:49-268) with every
// parameter set resident on the device.  A line-search trial is: one step + local prox + partial sums
// kernel, (column-coupled regularisers: psgd.hip's threshold passes and one more reduction pass), the forward pass of the
// trial set, the loss partials, and one finish kernel that adds every partial in workgroup order into a record of a few
// doubles.  That record is all that crosses to the host per trial; the branches of the three fit loops are taken here, on
// the host side of the library.  No floating-point atomics: every sum is a fixed tree, the same bits run to run.
#include <math.h>

#include <algorithm>

#include "fm_device.h"
#include "pgd.h"
#include "prox_dev.h"

namespace nfm {

enum { PGD_STEP = 0, PGD_REDUCE = 1 };
// a record slot (RS_*, pgd.h): {b_new, dot_b, viol_b, loss_sum}, then {dot, viol, sq, eval} per device block and for the
// linear part, then the column-wise SquaredL12 value per device block
enum { SLOT_TRIAL = 0, SLOT_AUX = 1, SLOT_BB = 2, N_SLOTS = 3 };

struct TrialArgs {
  ModelView M;  // geometry; P / w / sc: the set the trial writes (PGD_STEP) or the set that is measured (PGD_REDUCE)
  const double *oP, *ow, *osc;  // old_params
  const double *gP, *gw, *gsc;  // grads
  double eta, invP, invW, invB, lam;
  int32_t reg, reg_transpose, mode, G;
  double* partial;  // [nb + 1][G][4]
  double* colpart;  // [nb][G][Kp]  (column-wise SquaredL12)
  double* norms;    // [nb][da]     (SquaredL21)
  double* rec;      // the slot
};

// sums red[q][0 .. kBlock) for q < NQ with one fixed tree; the totals end in red[q][0]
template <int NQ>
__device__ __forceinline__ void block_tree(double (*red)[kBlock]) {
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
#pragma unroll
      for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + st];
    __syncthreads();
  }
}

// Params.step (model/params.nim:90-98) from old_params and grads into the trial set, the row-local prox (l1.nim:35-39,
// l21.nim:23-34, squaredl12.nim:161-162) in the same pass, and the partial sums of dot(new, grads) (params.nim:101-106),
// computeViol (utils.nim:5-17), |P|^2, |w|^2 and reg.eval.  grid (G, nb + 1): y < nb walks device block y, y == nb the
// linear term and the intercept.
template <int L>
__global__ __launch_bounds__(kBlock) void k_pgd_trial(TrialArgs a) {
  constexpr int R = kWave / L;
  __shared__ double red[6][kBlock];
  const ModelView& M = a.M;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int g = lane / L, l = lane % L, b = blockIdx.y;
  double dot = 0.0, viol = 0.0, sq = 0.0, ev = 0.0, cx = 0.0, cy = 0.0;
  if (b < M.nb) {
    const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * R;
    for (int64_t j0 = ((int64_t)blockIdx.x * kWavesPerBlock + wv) * R; j0 < M.da; j0 += stride) {  // uniform per wavefront
      const int64_t j = j0 + g;
      const bool act = j < M.da;  // inactive lanes keep taking part in the shuffles
      const size_t e = M.row(b, act ? j : 0) * M.Kp + 2 * l;
      double2 o = {0.0, 0.0}, gr = {0.0, 0.0}, p = {0.0, 0.0};
      if (act) {
        o = *reinterpret_cast<const double2*>(a.oP + e);
        gr = *reinterpret_cast<const double2*>(a.gP + e);
      }
      if (a.mode == PGD_STEP) {
        p.x = (o.x + -a.eta * gr.x) * a.invP;
        p.y = (o.y + -a.eta * gr.y) * a.invP;
        NFM_ROW_LOCAL_PROX(L, a.reg, a.reg_transpose, a.lam, p, act, l, a.norms[(size_t)b * M.da + j]);
        if (act) *reinterpret_cast<double2*>(M.P + e) = p;
      } else if (act) {
        p = *reinterpret_cast<const double2*>(M.P + e);
      }
      const double dx = p.x - o.x, dy = p.y - o.y;
      dot += p.x * gr.x + p.y * gr.y;
      viol += dx * dx + dy * dy;
      sq += p.x * p.x + p.y * p.y;
      if (a.reg == NFM_REG_L1) {
        ev += fabs(p.x) + fabs(p.y);
      } else if (a.reg == NFM_REG_L21 || a.reg == NFM_REG_SQUAREDL21) {
        const double nrm = sqrt(dev::row_sum<L>(p.x * p.x + p.y * p.y));
        if (l == 0) ev += nrm;
      } else if (a.reg_transpose) {
        cx += fabs(p.x);
        cy += fabs(p.y);
      } else {
        const double rs = dev::row_sum<L>(fabs(p.x) + fabs(p.y));
        if (l == 0) ev += rs * rs;
      }
    }
  } else {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < M.d; j += (int64_t)gridDim.x * kBlock) {
      const double ow = a.ow[j], gw = a.gw[j];
      double wn;
      if (a.mode == PGD_STEP) {
        wn = M.fit_linear ? (ow + -a.eta * gw) * a.invW : ow;  // params.nim:41-45,63-64
        M.w[j] = wn;
      } else {
        wn = M.w[j];
      }
      if (M.fit_linear) {
        dot += wn * gw;
        viol += (wn - ow) * (wn - ow);
      }
      sq += wn * wn;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const double ob = a.osc[SC_INTERCEPT], gb = a.gsc[SC_INTERCEPT];
      double bn;
      if (a.mode == PGD_STEP) {
        bn = ob;
        if (M.fit_intercept && M.fit_linear) bn += -a.eta * gb;  // params.nim:47 gates the step on grad.fitLinear
        if (M.fit_intercept) bn *= a.invB;                       // :65-66
        M.sc[SC_SCALE_P] = 1.0;
        M.sc[SC_SCALE_W] = 1.0;
        M.sc[SC_INTERCEPT] = bn;
      } else {
        bn = M.sc[SC_INTERCEPT];
      }
      a.rec[RS_B] = bn;
      a.rec[RS_DOTB] = M.fit_intercept ? bn * gb : 0.0;
      a.rec[RS_VIOLB] = M.fit_intercept ? (bn - ob) * (bn - ob) : 0.0;
    }
  }
  red[0][threadIdx.x] = dot;
  red[1][threadIdx.x] = viol;
  red[2][threadIdx.x] = sq;
  red[3][threadIdx.x] = ev;
  red[4][threadIdx.x] = cx;
  red[5][threadIdx.x] = cy;
  __syncthreads();
  if (a.colpart != nullptr && b < M.nb) {
    // thread (c, t), t < L: the lane groups hold factor pair t at threads q * L + t, added in q order
    for (int u = threadIdx.x; u < 2 * L; u += kBlock) {
      const int c = u / L, t = u % L;
      double acc = 0.0;
      for (int q = 0; q < kBlock / L; ++q) acc += red[4 + c][q * L + t];
      a.colpart[((size_t)b * a.G + blockIdx.x) * M.Kp + 2 * t + c] = acc;
    }
  }
  block_tree<4>(red);
  if (threadIdx.x < 4) a.partial[((size_t)b * a.G + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// sum_i loss(y_i, yPred_i) (pgd.nim:129-132), per-workgroup partials
__global__ __launch_bounds__(kBlock) void k_pgd_loss(const double* __restrict__ yhat, const double* __restrict__ y, int64_t n, int task,
                                                     int loss, double param, double* lpart) {
  __shared__ double red[1][kBlock];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    acc += dev::loss_value(loss, param, dev::target_of(y[i], task), yhat[i]);
  red[0][threadIdx.x] = acc;
  block_tree<1>(red);
  if (threadIdx.x == 0) lpart[blockIdx.x] = red[0][0];
}

struct FinArgs {
  const double* partial;  // [NY][G][4]
  const double* colpart;  // [nb][G][Kp] or NULL
  const double* lpart;    // [GL] or NULL
  double* rec;
  int32_t NY, G, nb, Kp, GL;
};

// one workgroup: every partial sum in workgroup order.  A wavefront owns an item: its lanes add the partials a wavefront
// apart, then one xor tree.
__global__ __launch_bounds__(kBlock) void k_pgd_finish(FinArgs f) {
  __shared__ double cs[kBlock];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int items = f.NY * 4 + (f.lpart != nullptr ? 1 : 0);
  for (int it = wv; it < items; it += kWavesPerBlock) {  // uniform per wavefront
    double acc = 0.0;
    if (it < f.NY * 4) {
      const int y = it / 4, q = it % 4;
      for (int g = lane; g < f.G; g += kWave) acc += f.partial[((size_t)y * f.G + g) * 4 + q];
    } else {
      for (int g = lane; g < f.GL; g += kWave) acc += f.lpart[g];
    }
    acc = dev::wave_sum(acc);
    if (lane == 0) f.rec[it < f.NY * 4 ? RS_PART + it : RS_LOSS] = acc;
  }
  if (f.colpart != nullptr) {  // squaredl12.nim:72-82, transpose: sum_s (sum_j |p_js|)^2
    for (int b = 0; b < f.nb; ++b) {
      double v = 0.0;
      for (int s = threadIdx.x; s < f.Kp; s += kBlock) {  // Kp <= 128: one round
        double col = 0.0;
        for (int g = 0; g < f.G; ++g) col += f.colpart[((size_t)b * f.G + g) * f.Kp + s];
        v = col * col;
      }
      __syncthreads();
      cs[threadIdx.x] = v;
      __syncthreads();
      if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < f.Kp; ++s) tot += cs[s];
        f.rec[RS_PART + f.NY * 4 + b] = tot;
      }
    }
  }
}

// nmapgd.getStepSize (nmapgd.nim:89-99) without s_params / r_params: ss = dot(s, s), sr = dot(s, r) with s = a - b and
// r = g - h, where Params.add leaves the linear term and the intercept alone unless fitLinear (params.nim:41-48).
// grid (G, 2): y == 0 the flat P arena (padding is zero in all four), y == 1 the linear term and the intercept
struct BbArgs {
  const double *aP, *bP, *gP, *hP, *aw, *bw, *gw, *hw, *asc, *bsc, *gsc, *hsc;
  int64_t nP, d;
  int32_t fit_linear, fit_intercept, G;
  double* partial;  // [2][G][4]
  double* rec;
};
__global__ __launch_bounds__(kBlock) void k_pgd_bb(BbArgs a) {
  __shared__ double red[2][kBlock];
  double ss = 0.0, sr = 0.0;
  if (blockIdx.y == 0) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < a.nP; e += (int64_t)gridDim.x * kBlock) {
      const double s = a.aP[e] + -1.0 * a.bP[e], r = a.gP[e] + -1.0 * a.hP[e];
      ss += s * s;
      sr += s * r;
    }
  } else {
    if (a.fit_linear)
      for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.d; j += (int64_t)gridDim.x * kBlock) {
        const double s = a.aw[j] + -1.0 * a.bw[j], r = a.gw[j] + -1.0 * a.hw[j];
        ss += s * s;
        sr += s * r;
      }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      double s = a.asc[SC_INTERCEPT], r = a.gsc[SC_INTERCEPT];
      if (a.fit_intercept && a.fit_linear) {
        s += -1.0 * a.bsc[SC_INTERCEPT];
        r += -1.0 * a.hsc[SC_INTERCEPT];
      }
      a.rec[RS_B] = a.fit_intercept ? s * s : 0.0;
      a.rec[RS_DOTB] = a.fit_intercept ? s * r : 0.0;
    }
  }
  red[0][threadIdx.x] = ss;
  red[1][threadIdx.x] = sr;
  block_tree<2>(red);
  if (threadIdx.x < 4) a.partial[((size_t)blockIdx.y * a.G + blockIdx.x) * 4 + threadIdx.x] = threadIdx.x < 2 ? red[threadIdx.x][0] : 0.0;
}

// fista.extrapolate (fista.nim:46-49): dst <- A; dst.add(B, cb); dst.add(C, cc)            (scale_first == 0)
// nmapgd.extrapolate (nmapgd.nim:133-138): dst <- A; dst *= ca; dst.add(B, cb); dst.add(C, cc)  (scale_first == 1)
// per element in that order; add and scale gate the linear term and the intercept as params.nim:41-48,61-66 do
struct MixArgs {
  double *dP, *dw, *dsc;
  const double *AP, *Aw, *Asc, *BP, *Bw, *Bsc, *CP, *Cw, *Csc;
  double ca, cb, cc;
  int64_t nP, d;
  int32_t scale_first, fit_linear, fit_intercept;
};
__global__ __launch_bounds__(kBlock) void k_pgd_mix(MixArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kBlock, t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int64_t e = t0; e < a.nP; e += stride) {
    double v = a.AP[e];
    if (a.scale_first) v *= a.ca;
    v += a.cb * a.BP[e];
    v += a.cc * a.CP[e];
    a.dP[e] = v;
  }
  for (int64_t j = t0; j < a.d; j += stride) {
    double v = a.Aw[j];
    if (a.fit_linear) {
      if (a.scale_first) v *= a.ca;
      v += a.cb * a.Bw[j];
      v += a.cc * a.Cw[j];
    }
    a.dw[j] = v;
  }
  if (t0 == 0) {
    double v = a.Asc[SC_INTERCEPT];
    if (a.scale_first && a.fit_intercept) v *= a.ca;
    if (a.fit_intercept && a.fit_linear) {
      v += a.cb * a.Bsc[SC_INTERCEPT];
      v += a.cc * a.Csc[SC_INTERCEPT];
    }
    a.dsc[SC_SCALE_P] = 1.0;
    a.dsc[SC_SCALE_W] = 1.0;
    a.dsc[SC_INTERCEPT] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
PgdState::~PgdState() {
  if (rec_h) (void)hipHostFree(rec_h);
}

int full_gradient(nfm_ctx* ctx, const CsrView& X, uint64_t ds_uid, const ModelView& M, const OptView& O_in, std::unique_ptr<Plan>& plan,
                  MbWork& W, double* gP, double* gw, double* gb, int64_t it, double* out2_host) {
  const int64_t n = X.n;
  OptView O = O_in;
  O.bsize = (double)n;  // one mini-batch holding every sample: coef = dloss / nSamples (pgd.nim:102)
  O.gradP = gP;
  O.gradw = gw;
  O.gradb = gb;
  W.use_graph = false;
  if (!plan || plan->ds_uid != ds_uid || plan->ds_nnz != X.nnz || plan->end != n || plan->n_aug != M.n_aug) {
    if (!plan) plan.reset(new Plan());
    const bool sort_by_count = M.Kp * (int)sizeof(double) >= 128;
    NFM_TRY(plan_build(ctx, X, M.n_aug, nullptr, 0, n, n, false, false, false, sort_by_count, plan.get()));
    plan->ds_uid = ds_uid;
    plan->ds_nnz = X.nnz;
  }
  return mb_fm_epoch(ctx, OPT_PSGD, X, M, O, *plan, W, it, out2_host);
}

namespace {

struct Red {  // one record slot, read on the host
  double b, dot, viol, psq, wsq, loss_sum;
  double ev[16];
};

struct Driver {
  nfm_ctx* ctx;
  const CsrView& X;
  uint64_t uid;
  ModelView M;  // the model handle's own arena: `params`
  PgdState* S;
  hipStream_t st;
  int64_t nPd;  // doubles of the P arena
  int no;       // the reference's orders

  Driver(nfm_ctx* c, const CsrView& x, uint64_t u, const ModelView& m, PgdState* s)
      : ctx(c), X(x), uid(u), M(m), S(s), st(c->stream), nPd((int64_t)m.nb * m.da * m.Kp), no(m.nb / m.kc) {}

  struct Ref {  // a parameter set by its three device pointers
    double *P, *w, *sc;
  };
  Ref ref(const PgdSet& s) const { return Ref{s.P(), s.w(), s.sc()}; }
  Ref params() const { return Ref{M.P, M.w, M.sc}; }
  ModelView view(Ref r) const {
    ModelView V = M;
    V.P = r.P;
    V.w = r.w;
    V.sc = r.sc;
    return V;
  }
  double* slot(int i) const { return S->rec.as<double>() + (size_t)i * S->slot; }
  const double* slot_h(int i) const { return S->rec_h + (size_t)i * S->slot; }
  bool coupled() const {
    return (S->cfg.reg == NFM_REG_SQUAREDL12 && S->cfg.reg_transpose) || S->cfg.reg == NFM_REG_SQUAREDL21;
  }
  int grid_rows() const {
    const int R = kWave / M.L;
    const int64_t need = std::max<int64_t>((std::max<int64_t>(M.da, M.d) + kWavesPerBlock * R - 1) / (kWavesPerBlock * R), 1);
    return (int)std::min<int64_t>(kPgdMaxBlocks, need);
  }

  int copy(Ref dst, Ref src) const {  // Params.`<-` (params.nim:79-82)
    if (nPd > 0) NFM_HIP_CHECK(hipMemcpyAsync(dst.P, src.P, sizeof(double) * nPd, hipMemcpyDeviceToDevice, st));
    if (M.d > 0) NFM_HIP_CHECK(hipMemcpyAsync(dst.w, src.w, sizeof(double) * M.d, hipMemcpyDeviceToDevice, st));
    NFM_HIP_CHECK(hipMemcpyAsync(dst.sc, src.sc, sizeof(double) * SC_COUNT, hipMemcpyDeviceToDevice, st));
    return NFM_OK;
  }

  void launch_trial(const TrialArgs& a) const {
    with_lanes(M.L, [&](auto L) {
      hipLaunchKernelGGL((k_pgd_trial<L()>), dim3((unsigned)a.G, (unsigned)(M.nb + 1)), dim3(kBlock), 0, st, a);
    });
  }
  TrialArgs trial_args(int slot_i, Ref nw, Ref old, Ref g, double eta, int mode) const {
    const PgdCfg& c = S->cfg;
    TrialArgs a{};
    a.M = view(nw);
    a.oP = old.P; a.ow = old.w; a.osc = old.sc;
    a.gP = g.P; a.gw = g.w; a.gsc = g.sc;
    a.eta = eta;
    a.invP = 1.0 / (1.0 + eta * c.beta);
    a.invW = 1.0 / (1.0 + eta * c.alpha);
    a.invB = 1.0 / (1.0 + eta * c.alpha0);
    a.lam = c.gamma * eta / (1.0 + eta * c.beta);  // pgd.nim:125
    a.reg = c.reg; a.reg_transpose = c.reg_transpose; a.mode = mode; a.G = grid_rows();
    a.partial = S->partial.as<double>();
    a.colpart = (c.reg == NFM_REG_SQUAREDL12 && c.reg_transpose) ? S->colpart.as<double>() : nullptr;
    a.norms = S->prox.as<double>();
    a.rec = slot(slot_i);
    return a;
  }
  void finish(int slot_i, const TrialArgs& a, bool with_loss, int GL) const {
    FinArgs f{a.partial, a.colpart, with_loss ? S->lpart.as<double>() : nullptr, slot(slot_i), M.nb + 1, a.G, M.nb, M.Kp, GL};
    hipLaunchKernelGGL(k_pgd_finish, dim3(1), dim3(kBlock), 0, st, f);
  }
  // the sums of (nw, old, g) as they are: dot(nw, g), computeViol(nw, old), the norms and reg.eval of nw
  int reduce(int slot_i, Ref nw, Ref old, Ref g) const {
    TimedLaunch tl(ctx, "pgd_trial");
    const TrialArgs a = trial_args(slot_i, nw, old, g, 0.0, PGD_REDUCE);
    launch_trial(a);
    finish(slot_i, a, false, 0);
    NFM_HIP_CHECK(hipGetLastError());
    return NFM_OK;
  }
  int loss_grid() const { return (int)std::min<int64_t>(kPgdMaxBlocks, (X.n + kBlock - 1) / kBlock); }
  // predictAll (pgd.nim:54-67) of a set and the loss partials
  int forward(Ref r) const {
    TimedLaunch tl(ctx, "pgd_forward");
    NFM_TRY(launch_predict(ctx, X, view(r), S->yhat.as<double>()));
    hipLaunchKernelGGL(k_pgd_loss, dim3((unsigned)loss_grid()), dim3(kBlock), 0, st, S->yhat.as<double>(), X.y, X.n, M.task, S->cfg.loss,
                       S->cfg.loss_param, S->lpart.as<double>());
    return NFM_OK;
  }
  // one line-search trial (pgd.nim:121-132): nw = prox(step(old, g, eta)), its forward pass, every sum into the slot
  int trial(Ref nw, Ref old, Ref g, double eta) const {
    TrialArgs a = trial_args(SLOT_TRIAL, nw, old, g, eta, PGD_STEP);
    {
      TimedLaunch tl(ctx, "pgd_trial");
      launch_trial(a);
      if (coupled()) {  // the threshold passes of psgd.hip, then the sums of what they left
        launch_prox_coupled(ctx, a.M, S->cfg.reg, a.lam, S->prox.as<double>());
        a.mode = PGD_REDUCE;
        launch_trial(a);
      }
    }
    NFM_TRY(forward(nw));
    TimedLaunch tl(ctx, "pgd_trial");
    finish(SLOT_TRIAL, a, true, loss_grid());
    NFM_HIP_CHECK(hipGetLastError());
    return NFM_OK;
  }
  int fetch() const {  // the only device-to-host traffic of an iteration besides the gradient pass's loss sum
    TimedLaunch tl(ctx, "pgd_wait");
    NFM_HIP_CHECK(hipMemcpyAsync(S->rec_h, S->rec.p, sizeof(double) * (size_t)N_SLOTS * S->slot, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    return NFM_OK;
  }
  Red read(int slot_i) const {
    const double* r = slot_h(slot_i);
    const PgdCfg& c = S->cfg;
    Red o{};
    o.b = r[RS_B];
    o.loss_sum = r[RS_LOSS];
    const double* lin = r + RS_PART + 4 * M.nb;
    for (int b = 0; b < M.nb; ++b) {
      const double* p = r + RS_PART + 4 * b;
      o.dot += p[0];
      o.viol += p[1];
      o.psq += p[2];
      o.ev[b / M.kc] += (c.reg == NFM_REG_SQUAREDL12 && c.reg_transpose) ? r[RS_PART + 4 * (M.nb + 1) + b] : p[3];
    }
    if (c.reg == NFM_REG_SQUAREDL21)  // squaredl21.nim:21-29: the square of the sum of the row norms
      for (int o_ = 0; o_ < no; ++o_) o.ev[o_] = o.ev[o_] * o.ev[o_];
    o.dot += lin[0];  // (the kernels gate the linear term and the intercept as Params.dot and computeViol do)
    o.viol += lin[1];
    o.wsq = lin[2];
    o.dot += r[RS_DOTB];
    o.viol += r[RS_VIOLB];
    return o;
  }
  // utils.regularization (utils.nim:56-59): norm(., 2)^2 squares the rounded square root
  double l2_terms(const Red& r) const {
    const PgdCfg& c = S->cfg;
    const double nw = sqrt(r.wsq), nP = sqrt(r.psq);
    double v = 0.5 * c.alpha0 * (r.b * r.b) + 0.5 * c.alpha * (nw * nw);
    v += 0.5 * c.beta * (nP * nP);
    return v;
  }
  // pgd.nim:144-146: reg.eval of order 0, once per order (kept); nmapgd.nim:122-123 walks the orders
  double reg_value(const Red& r, bool order0_only) const {
    double v = l2_terms(r);
    for (int o = 0; o < no; ++o) v += S->cfg.gamma * r.ev[order0_only ? 0 : o];
    return v;
  }

  int gradient(Ref at, const PgdSet& g, double* loss_sum) const {
    TimedLaunch tl(ctx, "pgd_grad");
    NFM_HIP_CHECK(hipMemsetAsync(g.buf.p, 0, g.buf.bytes, st));
    OptView O{};
    O.loss = S->cfg.loss;
    O.loss_param = S->cfg.loss_param;
    O.touch_cap = 1.0;
    O.eta0 = 1.0;
    O.reg = S->cfg.reg;
    O.reg_transpose = S->cfg.reg_transpose;
    double out2[2] = {0.0, 0.0};
    NFM_TRY(full_gradient(ctx, X, uid, view(at), O, S->plan, S->W, g.P(), g.w(), g.sc() + SC_INTERCEPT, 0, out2));
    *loss_sum = out2[0];
    return NFM_OK;
  }

  // pgd.linesearch (pgd.nim:106-146).  dot(old, grads) is formed once.  Returns (lossVal, regVal) and leaves the last trial's
  // record in SLOT_TRIAL.
  int linesearch_pgd(Ref nw, Ref old, const PgdSet& g, double old_loss_sum, int which, double* lossVal, double* regVal) const {
    const PgdCfg& c = S->cfg;
    const double nd = (double)X.n, oldLossVal = old_loss_sum / nd;
    NFM_TRY(reduce(SLOT_AUX, old, old, ref(g)));
    double eta = 1.0;
    int64_t it = 0;
    int trials = 0;
    Red r{};
    while (it < c.max_search || c.max_search <= 0) {
      NFM_TRY(trial(nw, old, ref(g), eta));
      NFM_TRY(fetch());
      ++trials;
      r = read(SLOT_TRIAL);
      const double dot_old = read(SLOT_AUX).dot;
      *lossVal = r.loss_sum / nd;
      double cond = r.dot - dot_old;
      cond += 0.5 * r.viol / eta;
      if ((*lossVal - oldLossVal) <= c.sigma * cond || eta < 1e-12) break;
      eta *= c.rho;
      ++it;
    }
    *regVal = reg_value(r, true);
    S->last.start[which] = 1.0;
    S->last.eta[which] = eta;
    S->last.trials[which] = (double)trials;
    S->last.viol = r.viol;
    return NFM_OK;
  }

  // nmapgd.linesearch (nmapgd.nim:102-130)
  int linesearch_nm(Ref nw, Ref old, const PgdSet& g, double eta0, double cref, int which, double* lossVal, double* regVal,
                    double* cond_out) const {
    const PgdCfg& c = S->cfg;
    const double nd = (double)X.n;
    double eta = eta0;
    int64_t it = 0;
    int trials = 0;
    while (it < c.max_search || c.max_search <= 0) {
      NFM_TRY(trial(nw, old, ref(g), eta));
      NFM_TRY(fetch());
      ++trials;
      const Red r = read(SLOT_TRIAL);
      *lossVal = r.loss_sum / nd;
      *regVal = reg_value(r, false);
      *cond_out = r.viol;
      if ((*lossVal + *regVal - cref) <= -c.sigma * r.viol || eta < 1e-12) break;
      eta *= c.rho;
      ++it;
    }
    S->last.start[which] = eta0;
    S->last.eta[which] = eta;
    S->last.trials[which] = (double)trials;
    return NFM_OK;
  }

  int mix(Ref dst, Ref A, Ref B, Ref C, bool scale_first, double ca, double cb, double cc) const {
    return launch_pgd_mix(ctx, M, PgdRef{dst.P, dst.w, dst.sc}, PgdRef{A.P, A.w, A.sc}, PgdRef{B.P, B.w, B.sc}, PgdRef{C.P, C.w, C.sc}, scale_first, ca, cb, cc);
  }

  // getStepSize (nmapgd.nim:89-99): |ss / sr|, 1 when either sum is exactly 0; the sums land in SLOT_BB with the next fetch
  int bb_launch(Ref a, Ref b, Ref g, Ref h) const {
    const int G = (int)std::min<int64_t>(kPgdMaxBlocks, std::max<int64_t>((std::max<int64_t>(nPd, M.d) + kBlock - 1) / kBlock, 1));
    BbArgs q{a.P, b.P, g.P, h.P, a.w, b.w, g.w, h.w, a.sc, b.sc, g.sc, h.sc, nPd, M.d, M.fit_linear, M.fit_intercept, G, S->partial.as<double>(), slot(SLOT_BB)};
    hipLaunchKernelGGL(k_pgd_bb, dim3((unsigned)G, 2), dim3(kBlock), 0, st, q);
    FinArgs f{S->partial.as<double>(), nullptr, nullptr, slot(SLOT_BB), 2, G, 0, 0, 0};
    hipLaunchKernelGGL(k_pgd_finish, dim3(1), dim3(kBlock), 0, st, f);
    NFM_HIP_CHECK(hipGetLastError());
    return NFM_OK;
  }
  double bb_read() const {
    const double* r = slot_h(SLOT_BB);
    double ss = r[RS_PART + 0], sr = r[RS_PART + 1];  // dot(P, P'), then w, then the intercept (params.nim:101-106)
    ss += r[RS_PART + 4 + 0];
    sr += r[RS_PART + 4 + 1];
    ss += r[RS_B];
    sr += r[RS_DOTB];
    if (ss == 0.0 || sr == 0.0) return 1.0;
    return fabs(ss / sr);
  }

  int epoch_pgd() const {  // pgd.nim:186-203
    double ls = 0.0;
    NFM_TRY(copy(ref(S->old), params()));
    NFM_TRY(gradient(params(), S->grads, &ls));
    S->last.branch = NFM_PGD_BRANCH_NONE;
    return linesearch_pgd(params(), ref(S->old), S->grads, ls, 0, &S->last.lossVal, &S->last.regVal);
  }

  int epoch_fista() const {  // fista.nim:99-127
    const double t = (sqrt(4 * (S->t * S->t) + 1.0) + 1.0) / 2.0;
    const double coef = (S->t - 1) / t;
    NFM_TRY(mix(ref(S->z), params(), params(), ref(S->old), false, 1.0, coef, -coef));
    NFM_TRY(copy(ref(S->old), ref(S->z)));
    double ls = 0.0, z_loss = 0.0, z_reg = 0.0;
    NFM_TRY(gradient(ref(S->z), S->grads, &ls));
    NFM_TRY(linesearch_pgd(ref(S->z), ref(S->old), S->grads, ls, 0, &z_loss, &z_reg));
    if ((z_loss + z_reg) <= (S->lossVal + S->regVal)) {  // Accept
      S->lossVal = z_loss;
      S->regVal = z_reg;
      NFM_TRY(copy(ref(S->old), params()));
      NFM_TRY(copy(params(), ref(S->z)));
      S->t = t;
      S->last.branch = NFM_PGD_BRANCH_ACCEPT;
    } else {  // Restart
      S->t = 1.0;
      S->last.branch = NFM_PGD_BRANCH_RESTART;
    }
    NFM_TRY(reduce(SLOT_AUX, params(), ref(S->old), ref(S->grads)));
    NFM_TRY(fetch());
    S->last.viol = read(SLOT_AUX).viol;
    S->last.lossVal = S->lossVal;
    S->last.regVal = S->regVal;
    return NFM_OK;
  }

  int epoch_nmapgd() const {  // nmapgd.nim:221-247
    const PgdCfg& c = S->cfg;
    const double nd = (double)X.n;
    const double t = (sqrt(4 * (S->t * S->t) + 1.0) + 1.0) / 2.0;
    NFM_TRY(mix(ref(S->y), ref(S->z), params(), ref(S->old_x), true, S->t / t, (t - 1) / t, -(S->t - 1) / t));
    NFM_TRY(copy(ref(S->old_x), params()));
    // epochZ (:141-157)
    double y_ls = 0.0;
    NFM_TRY(gradient(ref(S->y), S->grads, &y_ls));
    NFM_TRY(bb_launch(ref(S->y), ref(S->old_y), ref(S->grads), ref(S->old_y_grads)));
    NFM_TRY(reduce(SLOT_AUX, ref(S->y), ref(S->y), ref(S->grads)));
    NFM_TRY(fetch());
    const double step_z = bb_read();
    const Red ry = read(SLOT_AUX);
    double cz = y_ls / nd + l2_terms(ry);
    for (int o = 0; o < no; ++o) cz += c.gamma * ry.ev[o];
    double z_loss = 0.0, z_reg = 0.0, cond = 0.0;
    NFM_TRY(linesearch_nm(ref(S->z), ref(S->y), S->grads, step_z, std::max(cz, S->c), 0, &z_loss, &z_reg, &cond));
    double v_loss = INFINITY, v_reg = INFINITY;
    S->last.eta[1] = 0.0;
    S->last.trials[1] = 0.0;
    if ((z_loss + z_reg) > S->c - c.sigma * cond) {  // epochV (:160-171): params itself is the trial set
      double x_ls = 0.0, vcond = 0.0;
      NFM_TRY(gradient(params(), S->x_grads, &x_ls));
      NFM_TRY(bb_launch(params(), ref(S->old_y), ref(S->x_grads), ref(S->old_y_grads)));
      NFM_TRY(fetch());
      const double step_v = bb_read();
      NFM_TRY(linesearch_nm(params(), ref(S->old_x), S->x_grads, step_v, S->c, 1, &v_loss, &v_reg, &vcond));
    }
    double lossVal, regVal;
    if ((z_loss + z_reg) <= (v_loss + v_reg)) {
      lossVal = z_loss;
      regVal = z_reg;
      NFM_TRY(copy(params(), ref(S->z)));
      S->last.branch = NFM_PGD_BRANCH_Z;
    } else {
      lossVal = v_loss;
      regVal = v_loss;  // nmapgd.nim:244, kept: it feeds c below
      S->last.branch = NFM_PGD_BRANCH_V;
    }
    // updateCaches (:79-86)
    NFM_TRY(copy(ref(S->old_y), ref(S->y)));
    NFM_TRY(copy(ref(S->old_y_grads), ref(S->grads)));
    S->t = t;
    S->c = c.eta * S->c * S->q + lossVal + regVal;
    S->q = c.eta * S->q + 1;
    S->c /= S->q;
    NFM_TRY(reduce(SLOT_AUX, params(), ref(S->old_x), ref(S->grads)));
    NFM_TRY(fetch());
    S->last.viol = read(SLOT_AUX).viol;
    S->last.lossVal = lossVal;
    S->last.regVal = regVal;
    return NFM_OK;
  }
};

}  // namespace

int launch_pgd_mix(nfm_ctx* ctx, const ModelView& M, PgdRef dst, PgdRef A, PgdRef B, PgdRef C, bool scale_first, double ca, double cb, double cc) {
  const int64_t nPd = (int64_t)M.nb * M.da * M.Kp;
  MixArgs a{dst.P, dst.w, dst.sc, A.P, A.w, A.sc, B.P, B.w, B.sc, C.P, C.w, C.sc, ca, cb, cc, nPd, M.d, scale_first ? 1 : 0, M.fit_linear, M.fit_intercept};
  const int64_t need = std::max<int64_t>((std::max<int64_t>(nPd, M.d) + kBlock - 1) / kBlock, 1);
  hipLaunchKernelGGL(k_pgd_mix, dim3((unsigned)std::min<int64_t>(need, (int64_t)ctx->n_cu * 16)), dim3(kBlock), 0, ctx->stream, a);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

int launch_pgd_finish(nfm_ctx* ctx, const double* partial, int NY, int G, double* rec) {
  FinArgs f{partial, nullptr, nullptr, rec, NY, G, 0, 0, 0};
  hipLaunchKernelGGL(k_pgd_finish, dim3(1), dim3(kBlock), 0, ctx->stream, f);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

int pgd_alloc_set(nfm_ctx* ctx, const ModelView& M, PgdSet& s, bool zero) {
  const int64_t nPd = (int64_t)M.nb * M.da * M.Kp;
  s.bP = (sizeof(double) * (size_t)std::max<int64_t>(nPd, 2) + 255) / 256 * 256;
  s.bw = (sizeof(double) * (size_t)std::max<int64_t>(M.d, 1) + 255) / 256 * 256;
  NFM_TRY(s.buf.ensure(s.bP + s.bw + sizeof(double) * SC_COUNT));
  if (zero) {
    NFM_HIP_CHECK(hipMemsetAsync(s.buf.p, 0, s.buf.bytes, ctx->stream));
    const double one[2] = {1.0, 1.0};
    NFM_HIP_CHECK(hipMemcpyAsync(s.sc(), one, sizeof(one), hipMemcpyHostToDevice, ctx->stream));
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  return NFM_OK;
}

int pgd_begin_fit(nfm_ctx* ctx, const CsrView& X, uint64_t uid, uint64_t serial, const ModelView& M, bool warm_start, PgdState* S) {
  const PgdCfg& c = S->cfg;
  NFM_CHECK(X.n > 0, NFM_ERR_INVALID, "the dataset has no samples");
  const int64_t key = (((int64_t)M.nb * 1000003 + M.da) * 1000003 + M.Kp) * 1000003 + M.d;
  const bool reshaped = key != S->shape_key;
  S->n = X.n;
  Driver D(ctx, X, uid, M, S);
  // the record, its pinned twin and the partial sums
  S->slot = RS_PART + 4 * (M.nb + 1) + M.nb + 3;
  NFM_TRY(S->rec.ensure(sizeof(double) * (size_t)N_SLOTS * S->slot));
  NFM_HIP_CHECK(hipMemsetAsync(S->rec.p, 0, S->rec.bytes, ctx->stream));
  if (S->rec_h) (void)hipHostFree(S->rec_h);
  S->rec_h = nullptr;
  NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&S->rec_h), sizeof(double) * (size_t)N_SLOTS * S->slot));
  NFM_TRY(S->partial.ensure(sizeof(double) * 4 * (size_t)kPgdMaxBlocks * (size_t)std::max(M.nb + 1, 2)));
  NFM_TRY(S->colpart.ensure(sizeof(double) * (size_t)kPgdMaxBlocks * (size_t)std::max(M.nb, 1) * M.Kp));
  NFM_TRY(S->lpart.ensure(sizeof(double) * kPgdMaxBlocks));
  NFM_TRY(S->yhat.ensure(sizeof(double) * (size_t)X.n));
  NFM_TRY(S->prox.ensure(sizeof(double) * prox_scratch_doubles(M)));
  NFM_TRY(pgd_alloc_set(ctx, M, S->grads, true));
  if (c.algo != NFM_PGD_ALGO_NMAPGD) NFM_TRY(pgd_alloc_set(ctx, M, S->old, false));
  if (c.algo == NFM_PGD_ALGO_PGD) {
    // pgd.nim:164-180: nothing is carried
  } else if (c.algo == NFM_PGD_ALGO_FISTA) {  // fista.nim:84-98
    NFM_TRY(pgd_alloc_set(ctx, M, S->z, false));
    NFM_TRY(D.copy(D.ref(S->old), D.params()));
    NFM_TRY(D.copy(D.ref(S->z), D.params()));
    if (!warm_start) S->t = 0.0;
    S->lossVal = INFINITY;
    S->regVal = INFINITY;
  } else {  // nmapgd.initCaches (nmapgd.nim:49-76) and the initial c (:208-215)
    if (!warm_start) {
      S->t = 0.0;
      S->c = -1.0;
      S->q = 1.0;
    }
    if (S->t == 0.0 || reshaped || !S->z.buf.p) {
      NFM_TRY(pgd_alloc_set(ctx, M, S->z, true));
      NFM_TRY(pgd_alloc_set(ctx, M, S->old_y_grads, true));
      NFM_TRY(pgd_alloc_set(ctx, M, S->old_y, false));
      NFM_TRY(pgd_alloc_set(ctx, M, S->old_x, false));
      NFM_TRY(D.copy(D.ref(S->old_y), D.params()));
      NFM_TRY(D.copy(D.ref(S->old_x), D.params()));
    }
    NFM_TRY(pgd_alloc_set(ctx, M, S->y, true));
    NFM_TRY(pgd_alloc_set(ctx, M, S->x_grads, true));
    if (S->c < 0) {
      NFM_TRY(D.forward(D.params()));
      const TrialArgs a = D.trial_args(SLOT_TRIAL, D.params(), D.params(), D.ref(S->grads), 0.0, PGD_REDUCE);
      D.launch_trial(a);
      D.finish(SLOT_TRIAL, a, true, D.loss_grid());
      NFM_HIP_CHECK(hipGetLastError());
      NFM_TRY(D.fetch());
      const Red r = D.read(SLOT_TRIAL);
      const double lossVal = r.loss_sum / (double)X.n;
      S->c = lossVal + D.reg_value(r, false);
    }
  }
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  S->shape_key = key;
  S->fit_uid = uid;
  S->fit_serial = serial;
  S->fit_ready = true;
  S->last = PgdIter{};
  S->last.t = S->t;
  S->last.c = S->c;
  S->last.q = S->q;
  return NFM_OK;
}

int pgd_epoch(nfm_ctx* ctx, const CsrView& X, uint64_t uid, const ModelView& M, PgdState* S, double* loss_sum, double* viol_sum) {
  Driver D(ctx, X, uid, M, S);
  S->last.eta[0] = S->last.eta[1] = 0.0;
  S->last.trials[0] = S->last.trials[1] = 0.0;
  S->last.start[0] = S->last.start[1] = 0.0;
  int rc;
  if (S->cfg.algo == NFM_PGD_ALGO_PGD) rc = D.epoch_pgd();
  else if (S->cfg.algo == NFM_PGD_ALGO_FISTA) rc = D.epoch_fista();
  else rc = D.epoch_nmapgd();
  NFM_TRY(rc);
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  S->last.t = S->t;
  S->last.c = S->c;
  S->last.q = S->q;
  if (loss_sum) *loss_sum = S->last.lossVal * (double)X.n;
  if (viol_sum) *viol_sum = S->last.viol;
  return NFM_OK;
}

}  // namespace nfm
