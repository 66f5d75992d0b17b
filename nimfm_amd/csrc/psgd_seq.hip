// nimfm_amd/csrc/psgd_seq.hip -- PSGD (optimizer/psgd.nim:76-215) on the device: SGD in the reference's sample order with
// the sparsity regularisers L1 (regularizer/l1.nim:47-52,80-136) and L21 (regularizer/l21.nim:38-43,64-113), whose effect on
// the rows a sample does not touch is caught up lazily.  Prediction and derivatives are optimizer/sgd.nim:146-202.
//
// One persistent workgroup walks perm[begin .. end), thread s on factor s.  The staged row, the staging of the stored
// parameter rows, predictWithGrad and the factor sum are seq_step.h's, shared with k_sequential; what is here is PSGD's:
// the snapshot values beside the row (scalings[j], thresholds[j]; w caught up by scaling_w / scalings_w[j]), the lazy update,
// reg.step, updateCacheSGD, the intercept and linear steps, the due mask.  The table lives in LDS, or in global memory when it
// does not fit (rows of hundreds of entries): every thread touches its own column, the row norms of L21 are read across
// columns behind a barrier.  This path is latency-bound by construction: one sample is in flight.
//
// Unlike seq.hip there is NO global scale: the lazy hooks of the regularisers do not collapse into one factor (L1's
// threshold is gamma * scaling * (threshold - thresholds[j]) with the threshold advanced by eta / scaling BEFORE the step's
// scaling, l1.nim:103-110).  The stored P holds the reference's working values and the caches are the reference's:
// scalings / thresholds [d + nAug] (ONE pair serves all orders), scalings_w [d], and the scalars scaling, threshold, scaling_w.
//
// The two dense events -- the regulariser's cache reset (scaling < 1e-8) and the reset of w (scaling_w < 1e-9, psgd.nim:162-166)
// -- are grid-wide kernels of their own.  The persistent kernel stops after the sample that makes one due and writes the
// position it reached and which pass is due; psgd_seq_run launches the pass and relaunches from that position.  No kernel
// waits for another workgroup, a flag or the host: every launch does a bounded amount of work and returns.
//
// ONE DEPARTURE from the reference: L1's resetCacheSGD (l1.nim:113-126) is not a catch-up -- it divides by the snapshot,
// thresholds by gamma * threshold - thresholds[j] and multiplies by the threshold, after which the next steps overflow unless
// every parameter is zero already.  Here L1's reset applies lazyUpdateFinal's formula (l1.nim:89-100) to every row and then
// resets the caches: what finalize does, and what L21's own reset does (l21.nim:90-101).  DESIGN.md section 22.
#include "psgd_seq.h"

#include "fm_device.h"
#include "prox_dev.h"  // the device code's one soft threshold (regularizer/utils.nim:4-5)
#include "seq_step.h"  // the staged row, predictWithGrad and the launch of a one-workgroup kernel, shared with seq.hip

namespace nfm {

struct PsgdSeqArgs {
  CsrView X;
  ModelView M;
  OptView O;
  PsgdSeqView S;
  const int64_t* perm;
  int64_t begin, end, it0;
  int m_cap;
  double* scratch;  // the tables in global memory when they do not fit the LDS, else null
};

// doubles of the per-sample tables: dA and the staged rows [nb][m_cap][T] each, the row norms [nb][m_cap], values, linear
// weights, the two snapshot values [m_cap] each, and the indices [m_cap] (int64)
static size_t psgd_table_doubles(int nb, int m_cap, int T) { return 2 * (size_t)nb * m_cap * T + (size_t)nb * m_cap + 5 * (size_t)m_cap; }

template <int REG>
__global__ void k_psgd_seq(PsgdSeqArgs a) {
  extern __shared__ double lds[];
  const CsrView& X = a.X;
  const ModelView& M = a.M;
  const OptView& O = a.O;
  const PsgdSeqView& S = a.S;
  const int T = blockDim.x, tid = threadIdx.x;
  const int Kp = M.Kp, nb = M.nb, k = M.k, n_aug = M.n_aug, mc = a.m_cap;
  const bool act = tid < k;  // the padding s >= k stays 0
  double* red = lds;  // [T]
  double* base = a.scratch ? a.scratch : lds + T;
  const size_t n_tab = (size_t)nb * mc * T;
  double* dA = base;                     // [nb][mc][T] derivative
  double* Pl = dA + n_tab;               // [nb][mc][T] working parameter values of the sample's rows
  double* nrm = Pl + n_tab;              // [nb][mc]    L21: row norms
  double* vl = nrm + (size_t)nb * mc;    // [mc] values
  double* wl = vl + mc;                  // [mc] linear weights, caught up
  double* scl = wl + mc;                 // [mc] scalings[j]
  double* thl = scl + mc;                // [mc] thresholds[j]
  int64_t* jl = reinterpret_cast<int64_t*>(thl + mc);  // [mc] indices
  const seqstep::StagedRow row{jl, vl, wl, Pl, mc, T, tid};
  double scaling = S.sc[PS_SCALING], threshold = S.sc[PS_THRESHOLD], scaling_w = S.sc[PS_SCALING_W], loss_acc = S.sc[PS_LOSS];
  double b = M.sc[SC_INTERCEPT];
  const double beta = O.beta, gamma = O.gamma;
  int due = 0;
  int64_t pos = a.begin, it = a.it0;

  // L21: norm(P[j], 2) of every staged row (l21.nim:26), an in-order sum over s ascending by ONE thread per row -- across
  // both wavefronts when k > 64 -- and a correctly rounded square root
  auto row_norms = [&](int m_tot) {
    __syncthreads();
    for (int r = tid; r < nb * m_tot; r += T) {
      const int blk = r / m_tot, q = r - blk * m_tot;
      const double* pr = Pl + ((size_t)blk * mc + q) * T;
      double acc = 0.0;
      int s = 0;
      for (; s + 4 <= k; s += 4) {  // loaded ahead, added in order: ONE wait per group of loads in the ISA (else drop this)
        double v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v4[u] = pr[s + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += v4[u] * v4[u];
      }
      for (; s < k; ++s) acc += pr[s] * pr[s];
      nrm[(size_t)blk * mc + q] = sqrt(acc);
    }
    __syncthreads();
  };

  for (; pos < a.end && !due; ++pos, ++it) {
    const int64_t i = a.perm ? a.perm[pos] : pos;
    const int64_t q0 = X.indptr[i];
    const int m = (int)(X.indptr[i + 1] - q0);
    const int m_tot = m + n_aug;
    const double y = dev::target_of(X.y[i], M.task);
    const double itf = (double)it;

    // ---- stage the row; psgd.nim:124-125: w[j] *= scaling_w / scalings_w[j], unconditionally ----
    __syncthreads();  // the previous step is done with the tables, and what it stored is visible
    row.load_entries(X, q0, m, m_tot, [&](int q, int64_t jq) {
      scl[q] = S.scalings[jq];
      thl[q] = S.thresholds[jq];
      if (q < m) {
        const double wv = M.w[jq] * (scaling_w / S.scalings_w[jq]);
        wl[q] = wv;
        if (!M.fit_linear) M.w[jq] = wv;  // (fitLinear: the step below stores the row's weights)
      }
    });
    __syncthreads();
    if (act) row.load_rows(M, m_tot);

    // ---- reg.lazyUpdate(P[order]) over the row's features and the dummy features (psgd.nim:126-129) ----
    if (REG == NFM_REG_L1) {  // l1.nim:80-86
      if (act)
        for (int blk = 0; blk < nb; ++blk)
          for (int q = 0; q < m_tot; ++q) {
            const size_t e = ((size_t)blk * mc + q) * T + tid;
            double p = Pl[e];
            p *= scaling / scl[q];
            Pl[e] = dev::soft_threshold(p, gamma * scaling * (threshold - thl[q]));
          }
    } else {  // l21.nim:64-69
      row_norms(m_tot);
      if (act)
        for (int blk = 0; blk < nb; ++blk)
          for (int q = 0; q < m_tot; ++q) {
            const size_t e = ((size_t)blk * mc + q) * T + tid;
            const double thq = thl[q], sq = scl[q], norm = nrm[(size_t)blk * mc + q];  // (loads first: at most two waits per entry in the ISA, not four)
            double p = Pl[e];
            const double th = (threshold - thq) / sq;
            const double lam = th * gamma;
            if (norm > lam) p *= (1.0 - lam / norm);
            else p = 0.0;
            p *= scaling / sq;
            Pl[e] = p;
          }
    }

    // ---- predictWithGrad (optimizer/sgd.nim:191-202) ----
    double yh = b;
    for (int q = 0; q < m; ++q) yh += wl[q] * vl[q];
    for (int o = 0; o < nb; ++o) {
      double kv = 0.0, tot = 0.0;
      if (act) kv = seqstep::anova_order<dev::kMaxDeg, false>(row, o, M.deg_of(o), m_tot, dA);
      seqstep::factor_sum(red, tid, k, kv, o, /*kc=*/1, tot, yh);  // (psgd_seq_run takes kc == 1 only)
    }

    loss_acc += dev::loss_value(O.loss, O.loss_param, y, yh);  // psgd.nim:132, before the step
    const double dL = dev::loss_grad(O.loss, O.loss_param, y, yh);
    const double eta_w = dev::get_eta(O.sched, O.eta0, O.power, O.alpha, itf);
    const double eta_P = dev::get_eta(O.sched, O.eta0, O.power, beta, itf);
    const double eta_P_scaled = eta_P / (1.0 + eta_P * beta);

    // ---- reg.step per order (psgd.nim:141-145) ----
    if (REG == NFM_REG_L1) {  // l1.nim:129-136
      if (act)
        for (int blk = 0; blk < nb; ++blk)
          for (int q = 0; q < m_tot; ++q) {
            const size_t e = ((size_t)blk * mc + q) * T + tid;
            const double p = Pl[e];
            const double update = eta_P_scaled * (dL * dA[e] + beta * p);
            M.P[M.row(blk, jl[q]) * Kp + tid] = dev::soft_threshold(p - update, gamma * eta_P_scaled);
          }
    } else {  // l21.nim:105-113
      if (act)
        for (int blk = 0; blk < nb; ++blk)
          for (int q = 0; q < m_tot; ++q) {
            const size_t e = ((size_t)blk * mc + q) * T + tid;
            const double p = Pl[e];
            const double update = eta_P_scaled * (dL * dA[e] + beta * p);
            Pl[e] = p - update;
          }
      row_norms(m_tot);
      const double lam = eta_P_scaled * gamma;
      if (act)
        for (int blk = 0; blk < nb; ++blk)
          for (int q = 0; q < m_tot; ++q) {
            const double norm = nrm[(size_t)blk * mc + q];
            double p = Pl[((size_t)blk * mc + q) * T + tid];
            if (norm > lam) p *= (1.0 - lam / norm);
            else p = 0.0;
            M.P[M.row(blk, jl[q]) * Kp + tid] = p;
          }
    }
    // ---- reg.updateCacheSGD, once per sample (psgd.nim:146) ----
    if (REG == NFM_REG_L1) {  // l1.nim:103-110: the threshold advances with the scaling BEFORE the step
      const double eps = eta_P / (1 + eta_P * beta);
      threshold += eps / scaling;
      scaling *= (1 - eps * beta);
    } else {  // l21.nim:81-87: eta_P, not eta_P_scaled
      threshold += eta_P * scaling;
      scaling /= (1 + eta_P * beta);
    }
    // ---- intercept and linear term (psgd.nim:150-154, fit_linear.nim:41-47) ----
    if (M.fit_intercept) {
      const double eta_b = dev::get_eta(O.sched, O.eta0, O.power, O.alpha0, itf);
      const double update = eta_b * (dL + O.alpha0 * b);
      b -= update / (1.0 + eta_b * O.alpha0);
    }
    const double eta_lin = eta_w / (1.0 + eta_w * O.alpha);
    scaling_w /= (1.0 + eta_w * O.alpha);  // psgd.nim:157
    for (int q = tid; q < m_tot; q += T) {
      const int64_t jq = jl[q];
      S.scalings[jq] = scaling;
      S.thresholds[jq] = threshold;
      if (q < m) {
        if (M.fit_linear) {
          const double wj = wl[q];
          const double update = eta_lin * (dL * vl[q] + O.alpha * wj);
          M.w[jq] = wj - update;
        }
        S.scalings_w[jq] = scaling_w;  // psgd.nim:158-159
      }
    }
    // ---- the dense events: the launch ends here and the host loop runs them (psgd.nim:162-167) ----
    if (M.fit_linear && scaling_w < 1e-9) due |= PSGD_DUE_W;
    if (scaling < 1e-8) due |= PSGD_DUE_CACHE;
  }

  __syncthreads();
  if (tid == 0) {
    S.sc[PS_SCALING] = scaling;
    S.sc[PS_THRESHOLD] = threshold;
    S.sc[PS_SCALING_W] = scaling_w;
    S.sc[PS_LOSS] = loss_acc;
    M.sc[SC_INTERCEPT] = b;
    S.ctl[0] = pos;
    S.ctl[1] = due;
  }
}

// ---- the dense passes ----
// w *= scaling_w; w /= scalings_w (psgd.nim:63-66 in finalize, :162-166 as the reset); the snapshots become `snap`
// (finalize: scaling_w itself, the reset: 1).  The scalar is only read here; k_psgd_set_scalars writes it afterwards.
__global__ void k_psgd_w_catchup(ModelView M, PsgdSeqView S, int reset) {
  const double sw = S.sc[PS_SCALING_W];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M.d; j += stride) {
    double w = M.w[j];
    w *= sw;
    w /= S.scalings_w[j];
    M.w[j] = w;
    S.scalings_w[j] = reset ? 1.0 : sw;
  }
}

// lazyUpdateFinal (l1.nim:89-96, l21.nim:72-78) on every row of every order; the caches are reset by the launches behind it.
// L1: one thread per element.  L21: one thread per row -- the norm is the in-order sum over s ascending.
template <int REG>
__global__ void k_psgd_lazy_final(ModelView M, PsgdSeqView S, double gamma) {
  const double scaling = S.sc[PS_SCALING], threshold = S.sc[PS_THRESHOLD];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t rows = (int64_t)M.nb * M.da;
  if (REG == NFM_REG_L1) {
    for (int64_t e = t0; e < rows * M.Kp; e += stride) {
      const int64_t r = e / M.Kp;
      const int s = (int)(e - r * M.Kp);
      if (s >= M.k) continue;
      const int64_t j = r % M.da;
      double p = M.P[e];
      p *= scaling / S.scalings[j];
      M.P[e] = dev::soft_threshold(p, gamma * scaling * (threshold - S.thresholds[j]));
    }
  } else {
    for (int64_t r = t0; r < rows; r += stride) {
      const int64_t j = r % M.da;
      double* row = M.P + (size_t)r * M.Kp;
      const double sj = S.scalings[j];
      const double th = (threshold - S.thresholds[j]) / sj;
      const double lam = th * gamma;
      double acc = 0.0;
      for (int s = 0; s < M.k; ++s) acc += row[s] * row[s];
      const double norm = sqrt(acc);
      const double f = scaling / sj;
      for (int s = 0; s < M.k; ++s) {
        double p = row[s];
        if (norm > lam) p *= (1.0 - lam / norm);
        else p = 0.0;
        p *= f;
        row[s] = p;
      }
    }
  }
}

__global__ void k_psgd_set_scalars(PsgdSeqView S, int reset_w, int reset_cache) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (reset_w) S.sc[PS_SCALING_W] = 1.0;
    if (reset_cache) {
      S.sc[PS_SCALING] = 1.0;
      S.sc[PS_THRESHOLD] = 0.0;
    }
  }
}

static unsigned dense_blocks(int64_t work) {
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 16) blocks = 256 * 16;
  return (unsigned)blocks;
}

static int launch_w_catchup(nfm_ctx* ctx, const ModelView& M, PsgdSeqState* S, bool reset) {
  TimedLaunch tl(ctx, "psgd_seq_dense");
  hipLaunchKernelGGL(k_psgd_w_catchup, dim3(dense_blocks(M.d)), dim3(kBlock), 0, ctx->stream, M, S->v, reset ? 1 : 0);
  NFM_HIP_CHECK(hipGetLastError());
  if (reset) {
    hipLaunchKernelGGL(k_psgd_set_scalars, dim3(1), dim3(kWave), 0, ctx->stream, S->v, 1, 0);
    NFM_HIP_CHECK(hipGetLastError());
  }
  return NFM_OK;
}

// lazyUpdateFinal, and with reset_caches the reset of the regulariser's caches behind it: the cache reset of the fit loop (see
// the head of this file) and L1's lazyUpdateFinal, which ends with it (l1.nim:97-100).  L21's lazyUpdateFinal leaves its
// caches as they are (l21.nim:72-78): kept as written, so a fit that goes on after a callback's finalize catches the same
// rows up again, as the reference does.
static int launch_lazy_final(nfm_ctx* ctx, const ModelView& M, const OptView& O, PsgdSeqState* S, bool reset_caches) {
  {
    TimedLaunch tl(ctx, "psgd_seq_dense");
    const int64_t rows = (int64_t)M.nb * M.da;
    if (O.reg == NFM_REG_L1)
      hipLaunchKernelGGL(k_psgd_lazy_final<NFM_REG_L1>, dim3(dense_blocks(rows * M.Kp)), dim3(kBlock), 0, ctx->stream, M, S->v, O.gamma);
    else
      hipLaunchKernelGGL(k_psgd_lazy_final<NFM_REG_L21>, dim3(dense_blocks(rows)), dim3(kBlock), 0, ctx->stream, M, S->v, O.gamma);
    NFM_HIP_CHECK(hipGetLastError());
    if (!reset_caches) return NFM_OK;
    hipLaunchKernelGGL(k_psgd_set_scalars, dim3(1), dim3(kWave), 0, ctx->stream, S->v, 0, 1);
    NFM_HIP_CHECK(hipGetLastError());
  }
  NFM_TRY(launch_fill(ctx, S->v.scalings, S->da, 1.0));
  NFM_TRY(launch_fill(ctx, S->v.thresholds, S->da, 0.0));
  return NFM_OK;
}

int psgd_seq_alloc(nfm_ctx* ctx, const ModelView& M, PsgdSeqState* S) {
  auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t b_da = pad(sizeof(double) * (size_t)M.da), b_d = pad(sizeof(double) * (size_t)(M.d > 0 ? M.d : 1));
  const size_t b_sc = pad(sizeof(double) * PS_COUNT + sizeof(int64_t) * 2);
  NFM_TRY(S->arena.alloc(2 * b_da + b_d + b_sc));
  NFM_HIP_CHECK(hipMemsetAsync(S->arena.p, 0, S->arena.bytes, ctx->stream));
  char* p = S->arena.as<char>();
  S->v.scalings = reinterpret_cast<double*>(p);
  S->v.thresholds = reinterpret_cast<double*>(p + b_da);
  S->v.scalings_w = reinterpret_cast<double*>(p + 2 * b_da);
  S->v.sc = reinterpret_cast<double*>(p + 2 * b_da + b_d);
  S->v.ctl = reinterpret_cast<int64_t*>(S->v.sc + PS_COUNT);
  S->d = M.d;
  S->da = M.da;
  S->fit_ready = false;
  return NFM_OK;
}

int psgd_seq_begin_fit(nfm_ctx* ctx, const ModelView& M, PsgdSeqState* S) {
  NFM_CHECK(S->arena.p && S->d == M.d && S->da == M.da, NFM_ERR_INVALID, "the optimizer's caches do not belong to this model");
  NFM_TRY(launch_fill(ctx, S->v.scalings, S->da, 1.0));
  NFM_TRY(launch_fill(ctx, S->v.thresholds, S->da, 0.0));
  NFM_TRY(launch_fill(ctx, S->v.scalings_w, S->d, 1.0));
  const double sc[PS_COUNT] = {1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  NFM_HIP_CHECK(hipMemcpyAsync(S->v.sc, sc, sizeof(sc), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (sc is a stack array)
  S->cache_resets = S->w_resets = 0;
  return NFM_OK;
}

int psgd_seq_run(nfm_ctx* ctx, const CsrView& X, const ModelView& M, const OptView& O, PsgdSeqState* S, const int64_t* perm_dev, int64_t begin,
                 int64_t end, int64_t it0, int m_cap, double* loss_sum) {
  NFM_CHECK(M.kind == NFM_KIND_FM && M.kc == 1 && M.Kp <= 128, NFM_ERR_UNSUPPORTED, "PSGD supports a FactorizationMachine with n_components <= 128");
  NFM_CHECK(M.degree <= dev::kMaxDeg, NFM_ERR_UNSUPPORTED, "PSGD supports degree <= %d", dev::kMaxDeg);
  NFM_CHECK(O.reg == NFM_REG_L1 || O.reg == NFM_REG_L21, NFM_ERR_UNSUPPORTED, "PSGD on the device takes L1 or L21");
  if (m_cap < 1) m_cap = 1;
  int T = ((M.Kp + kWave - 1) / kWave) * kWave;
  if (T < kWave) T = kWave;
  const SeqTable tab = seq_sample_table(T, sizeof(double) * psgd_table_doubles(M.nb, m_cap, T));
  const size_t lds_bytes = tab.lds_bytes;
  double* scratch = nullptr;
  NFM_TRY(seqstep::place_sample_table(ctx, tab.in_lds, tab.table_bytes, &scratch));
  NFM_HIP_CHECK(hipMemsetAsync(S->v.sc + PS_LOSS, 0, sizeof(double), ctx->stream));  // the running loss of this call
  PsgdSeqCursor cur(begin, end, it0);
  while (!cur.done()) {
    PsgdSeqArgs a{X, M, O, S->v, perm_dev, cur.pos, end, cur.it(), m_cap, scratch};
    NFM_TRY(seqstep::launch_one_workgroup(ctx, "psgd_seq", O.reg == NFM_REG_L1 ? k_psgd_seq<NFM_REG_L1> : k_psgd_seq<NFM_REG_L21>, T, lds_bytes, a));
    int64_t ctl[2] = {0, 0};
    NFM_HIP_CHECK(hipMemcpyAsync(ctl, S->v.ctl, sizeof(ctl), hipMemcpyDeviceToHost, ctx->stream));
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    NFM_CHECK(cur.advance(ctl[0], ctl[1]), NFM_ERR_HIP, "PSGD: the kernel reported position %lld (mask %lld) for the range [%lld,%lld)",
              (long long)ctl[0], (long long)ctl[1], (long long)cur.pos, (long long)end);
    if (ctl[1] & PSGD_DUE_W) {
      NFM_TRY(launch_w_catchup(ctx, M, S, /*reset=*/true));
      ++S->w_resets;
    }
    if (ctl[1] & PSGD_DUE_CACHE) {
      NFM_TRY(launch_lazy_final(ctx, M, O, S, /*reset_caches=*/true));
      ++S->cache_resets;
    }
  }
  double ls = 0.0;
  NFM_HIP_CHECK(hipMemcpyAsync(&ls, S->v.sc + PS_LOSS, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (loss_sum) *loss_sum = ls;
  return NFM_OK;
}

int psgd_seq_finalize(nfm_ctx* ctx, const ModelView& M, const OptView& O, PsgdSeqState* S) {
  if (M.fit_linear) NFM_TRY(launch_w_catchup(ctx, M, S, /*reset=*/false));
  NFM_TRY(launch_lazy_final(ctx, M, O, S, /*reset_caches=*/O.reg == NFM_REG_L1));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return NFM_OK;
}

}  // namespace nfm
