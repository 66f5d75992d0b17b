// nimfm_amd/csrc/pbcd.hip -- proximal block coordinate descent for sparse FactorizationMachines (newPBCD,
// optimizer/pbcd.nim:112-329 at maxSearch = 0) on CD's schedules.
//
// The reference steps a feature's whole row P[j, 0..k) at once: one walk of the schedule per order and iteration where CD
// and PCD walk it once per component.  The state is anova's table A [degree + 1][n][k] and its derivative dA [degree][n][k]
// for every component (pbcd.nim:233-236) beside CD's yPred.  One wavefront steps one feature.  In the passes over the
// column its lanes are the components: lane s walks the column in storage order and keeps its own component's sums, so
// every sum over a column is in the reference's order without a chain across lanes.  The sums over the components
// (sum(invStepSizes), the norms, norm(delta, 1)) are an in-order chain over the lanes, and dot(delta, dA[degree - 1, i])
// is formed by a lane per sample over the stored dA row, ascending s.  Components beyond 64 are further blocks of lanes:
// addressing only, the sums continue across the blocks.
//
// L1 (l1.nim:31-33) and L21 (l21.nim:25-29) read nothing but the feature's own row -- with maxSearch = 0 their running
// `value` is read by the verbose line alone -- and run CD's level schedule.  SquaredL21 (squaredl21.nim:32-43,90-101) reads
// norms[j] and the running cache = sum(norms): the run schedule in three phases, (a) gradients and the pre-prox row, (b)
// the chain in ascending j, (c) the synchronisations.  OmegaCS (omegacs.nim:31-85) is a second chain on the same schedule, at
// any degree: its running state is the ANOVA polynomials of every row's norm, cache[0 .. deg], and the ones without the
// current row, dcache[0 .. deg].  The intercept, the w sweep and the loss sum are cd.hip's.
#include <math.h>

#include <algorithm>

#include "cd.h"
#include "cd_dev.h"
#include "fm_device.h"

namespace nfm {
using namespace dev;

namespace {

struct PbDev {
  double* P;  // the model's table, through at()
  int64_t bs, rs;
  int32_t Kp, kb, kc, nc;  // kb factors per device block, kc blocks per order, nc components
  int32_t o, deg, reg, pad_;
  int64_t da, vbase;  // features with the dummies; index in `out` of this order's feature 0
  double* A;          // [degree + 1][n][nc]
  double* dA;         // [degree][n][nc]
  double* row;        // [da][nc]: grad, then the pre-prox row
  double* delta;      // [da][nc]: old - new
  double* inv;        // [da] each: invStepSize,
  double* pnorm;      //   the pre-prox row's norm (SquaredL21, OmegaCS),
  double* scale;      //   the chain's factor on the pre-prox row (0: the row is set to zero),
  double* norms;      //   the chained regularisers' norms[j]
  double* chain;      // chain[0]: SquaredL21's cache; OmegaCS: cache[0 .. kCdMaxDeg], then dcache[0 .. kCdMaxDeg] (CsState)
  const int64_t* roff;
  double beta, gamma, nf;  // UNSCALED strengths (pbcd.nim:138,147,154), float(nSamples)
  __device__ double& at(int s, int64_t j) const { return P[(size_t)(((int64_t)o * kc + s / kb) * bs + j * rs) * Kp + s % kb]; }
  __device__ double* tab(double* T, int t, int64_t n, int64_t i) const { return T + ((size_t)t * n + i) * nc; }
};

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// linear(X, w) (per sample, ascending j) + intercept (pbcd.nim:261-262)
__global__ void k_pb_linear(CdDev D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  double acc = 0.0;
  for (int64_t q = D.rptr[i]; q < D.rptr[i + 1]; ++q) acc += D.rval[q] * D.w[D.ridx[q]];
  acc += D.sc[SC_INTERCEPT];
  D.yp[i] = acc;
}

// precomputeAnova (pbcd.nim:61-77): always the general recursion, product order (A * val) * P; per (sample, component)
// in ascending j, the dummy features last
__global__ void k_pb_anova(CdDev D, PbDev B) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= D.n * B.nc) return;
  const int64_t i = t / B.nc;
  const int s = (int)(t % B.nc);
  const int deg = B.deg;
  double A[kCdMaxDeg + 1];
  A[0] = 1.0;
  for (int g = 1; g <= deg; ++g) A[g] = 0.0;
  const int64_t q0 = D.rptr[i], q1 = D.rptr[i + 1], nd = B.da - D.d;
  for (int64_t q = q0; q < q1 + nd; ++q) {
    const bool dummy = q >= q1;
    const int64_t j = dummy ? D.d + (q - q1) : D.ridx[q];
    const double v = dummy ? 1.0 : D.rval[q];
    const double p = B.at(s, j);
    for (int g = 0; g < deg; ++g) A[deg - g] += A[deg - g - 1] * v * p;
  }
  for (int g = 0; g <= deg; ++g) B.tab(B.A, g, D.n, i)[s] = A[g];
}

// yPred[i] += A[degree - order, i, s], s ascending (pbcd.nim:267-269)
__global__ void k_pb_add_top(CdDev D, PbDev B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const double* top = B.tab(B.A, B.deg, D.n, i);
  double acc = D.yp[i];
  for (int s = 0; s < B.nc; ++s) acc += top[s];
  D.yp[i] = acc;
}

// v of lanes 0 .. cnt-1 added to acc one after the other: the reference's ascending sum over the components
__device__ __forceinline__ double lanes_in_order(double acc, double v, int cnt) {
  for (int l = 0; l < cnt; ++l) acc += shfl_d(v, l);
  return acc;
}

// dA[0 .. deg)[i][s] of one column entry (pbcd.nim:49-58,126-128) into the table; -> dA[deg - 1][i][s]
__device__ __forceinline__ double pb_derivative(const PbDev& B, int64_t n, int64_t i, int s, double v, double pjs) {
  if (B.deg == 2) {
    const double t = v * (B.tab(B.A, 1, n, i)[s] - v * pjs);
    B.tab(B.dA, 1, n, i)[s] = t;
    return t;
  }
  double prev = v;
  B.tab(B.dA, 0, n, i)[s] = v;
  for (int g = 1; g < B.deg; ++g) {
    prev = v * (B.tab(B.A, g, n, i)[s] - pjs * prev);
    B.tab(B.dA, g, n, i)[s] = prev;
  }
  return prev;
}

// invStepSize from sum(invStepSizes) (pbcd.nim:145-148)
__device__ __forceinline__ double pb_inv(const CdDev& D, const PbDev& B, double invsum) {
  double inv = invsum * D.mu / B.nf;
  inv += B.beta;
  return inv < 1e-12 ? 1e-12 : inv;
}

// update (pbcd.nim:119-148) of one feature, one wavefront, lanes = components: dA of the column, grad[s] into row[j][s],
// -> invStepSize
__device__ __forceinline__ double pb_grad(const CdDev& D, const PbDev& B, int64_t j, int lane) {
  const int64_t c0 = D.cptr[j], c1 = D.cptr[j + 1];
  double invsum = 0.0;
  if (B.nc <= kWave / 2) {
    // few components: the wavefront holds G = 64 / w samples at a time, w lanes (a power of two >= nc) each; the terms
    // of the G samples are added in column order, as CD's lanes are (cd.hip: cd_grad)
    int w = 1;
    while (w < B.nc) w <<= 1;
    const int G = kWave / w, slot = lane / w, s = lane % w;
    const bool act = s < B.nc;
    const double pjs = act ? B.at(s, j) : 0.0;
    double g = 0.0, iv = 0.0;
    for (int64_t base = c0; base < c1; base += G) {
      const int64_t q = base + slot;
      double t1 = 0.0, t2 = 0.0;
      if (q < c1 && act) {
        const int64_t i = D.crow[q];
        const double t = pb_derivative(B, D.n, i, s, D.cval[q], pjs);
        t1 = dloss_at(D, i) * t;
        t2 = t * t;
      }
      const int cnt = (int)min((int64_t)G, c1 - base);
      for (int l = 0; l < cnt; ++l) {
        g += shfl_d(t1, l * w + s);
        iv += shfl_d(t2, l * w + s);
      }
    }
    if (act && slot == 0) {
      g /= B.nf;
      g += B.beta * pjs;
      B.row[(size_t)j * B.nc + s] = g;
    }
    return pb_inv(D, B, lanes_in_order(0.0, iv, B.nc));
  }
  for (int sb = 0; sb < B.nc; sb += kWave) {
    const int s = sb + lane;
    const bool act = s < B.nc;
    const double pjs = act ? B.at(s, j) : 0.0;
    double g = 0.0, iv = 0.0;
    for (int64_t q = c0; q < c1; ++q) {
      const int64_t i = D.crow[q];
      const double dl = dloss_at(D, i);
      if (act) {
        const double t = pb_derivative(B, D.n, i, s, D.cval[q], pjs);
        g += dl * t;
        iv += t * t;
      }
    }
    if (act) {
      g /= B.nf;
      g += B.beta * pjs;
      B.row[(size_t)j * B.nc + s] = g;
    }
    invsum = lanes_in_order(invsum, iv, min(kWave, B.nc - sb));
  }
  return pb_inv(D, B, invsum);
}

// the pre-prox row P[j] - grad / invStepSize (pbcd.nim:150-152), divided by 1 + 2 lam when `div` (squaredl21.nim:34-35),
// into row[j]; -> its norm(., 2) when `want_norm`
__device__ __forceinline__ double pb_pre(const PbDev& B, int64_t j, int lane, double inv, bool div, double lam, bool want_norm) {
  double sq = 0.0;
  for (int sb = 0; sb < B.nc; sb += kWave) {
    const int s = sb + lane;
    double u = 0.0;
    if (s < B.nc) {
      u = B.at(s, j) - B.row[(size_t)j * B.nc + s] / inv;
      if (div) u /= (1 + 2 * lam);
      B.row[(size_t)j * B.nc + s] = u;
    }
    if (want_norm) sq = lanes_in_order(sq, u * u, min(kWave, B.nc - sb));
  }
  return want_norm ? sqrt(sq) : 0.0;
}

// the new row is `factor` times the pre-prox row (factor 0: zero; L1: its soft threshold at lam): P[j], delta = old - new
// and norm(delta, 1) (pbcd.nim:154-157,191)
__device__ __forceinline__ void pb_apply(const CdDev& D, const PbDev& B, int64_t j, int lane, bool l1, double lam, double factor) {
  double viol = 0.0;
  for (int sb = 0; sb < B.nc; sb += kWave) {
    const int s = sb + lane;
    double dl = 0.0;
    if (s < B.nc) {
      const double u = B.row[(size_t)j * B.nc + s], old = B.at(s, j);
      const double pn = l1 ? soft_threshold(u, lam) : (factor == 0.0 ? 0.0 : u * factor);
      B.at(s, j) = pn;
      dl = -pn + old;
      B.delta[(size_t)j * B.nc + s] = dl;
    }
    viol = lanes_in_order(viol, fabs(dl), min(kWave, B.nc - sb));
  }
  if (lane == 0) D.out[B.vbase + j] = viol;
}

// one sample of a column: yPred[i] -= dot(delta, dA[deg - 1, i]) (ascending s), then A (pbcd.nim:184-206: degree 2
// A[1] -= val * delta, else A[g] -= dA[g - 1] * delta for g < degree; A[degree] stays)
__device__ __forceinline__ void pb_sync_sample(const CdDev& D, const PbDev& B, const double* dl, int64_t i, double v) {
  const double* top = B.tab(B.dA, B.deg - 1, D.n, i);
  double dot = 0.0;
  for (int s = 0; s < B.nc; ++s) dot += dl[s] * top[s];
  D.yp[i] -= dot;
  if (B.deg == 2) {
    double* A1 = B.tab(B.A, 1, D.n, i);
    for (int s = 0; s < B.nc; ++s) A1[s] -= v * dl[s];
  } else {
    for (int g = 1; g < B.deg; ++g) {
      double* Ag = B.tab(B.A, g, D.n, i);
      const double* dg = B.tab(B.dA, g - 1, D.n, i);
      for (int s = 0; s < B.nc; ++s) Ag[s] -= dg[s] * dl[s];
    }
  }
}

// the synchronisation of one feature, one wavefront, a lane per sample of the column.  dA and delta were written by the
// other lanes of this wavefront (or an earlier kernel / before a workgroup barrier): the fence orders them.
__device__ __forceinline__ void pb_sync(const CdDev& D, const PbDev& B, int64_t j, int lane) {
  __threadfence_block();
  const double* dl = B.delta + (size_t)j * B.nc;
  const int64_t c1 = D.cptr[j + 1];
  for (int64_t q = D.cptr[j] + lane; q < c1; q += kWave) pb_sync_sample(D, B, dl, D.crow[q], D.cval[q]);
}

// L1 / L21: the whole step of one feature, one wavefront
__device__ __forceinline__ void pb_feature(const CdDev& D, const PbDev& B, int64_t j, int lane) {
  const double inv = pb_grad(D, B, j, lane);
  const double lam = B.gamma / inv;
  const bool l1 = B.reg == NFM_REG_L1;
  const double nrm = pb_pre(B, j, lane, inv, false, 0.0, !l1);
  const double factor = l1 ? 1.0 : (nrm > lam ? 1.0 - lam / nrm : 0.0);  // l21.nim:25-29
  pb_apply(D, B, j, lane, l1, lam, factor);
  pb_sync(D, B, j, lane);
}

__global__ void __launch_bounds__(kBlock) k_pb_level(CdDev D, PbDev B, const int32_t* order, int64_t f0, int64_t f1) {
  const int64_t f = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (f >= f1) return;
  pb_feature(D, B, order[f], threadIdx.x % kWave);
}

__global__ void __launch_bounds__(kNarrowBlock) k_pb_levels(CdDev D, PbDev B, const int32_t* order, const int64_t* goff, int64_t g0,
                                                            int64_t g1) {
  const int wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t f1 = goff[g + 1];
    for (int64_t f = goff[g] + wv; f < f1; f += kNarrowWaves) pb_feature(D, B, order[f], lane);
    __syncthreads();
  }
}

// ---- SquaredL21: the run schedule ----
// computeCacheBCD (squaredl21.nim:90-94): norms[j] = norm(P[j], 2), cache = sum(norms) in ascending j; one wavefront
__global__ void __launch_bounds__(kWave) k_pb_norms(PbDev B) {
  const int lane = threadIdx.x;
  double cache = 0.0;
  for (int64_t base = 0; base < B.da; base += kWave) {
    const int64_t j = base + lane;
    double nm = 0.0;
    if (j < B.da) {
      double sq = 0.0;
      for (int s = 0; s < B.nc; ++s) {
        const double p = B.at(s, j);
        sq += p * p;
      }
      nm = sqrt(sq);
      B.norms[j] = nm;
    }
    cache = lanes_in_order(cache, nm, (int)min((int64_t)kWave, B.da - base));
  }
  if (lane == 0) B.chain[0] = cache;
}

// phase (a) of one feature: nothing here reads the chain.  CS: OmegaCS, whose pre-prox row is not divided
template <bool CS>
__device__ __forceinline__ void pb_sq_pre(const CdDev& D, const PbDev& B, int64_t j, int lane) {
  const double inv = pb_grad(D, B, j, lane);
  const double nrm = pb_pre(B, j, lane, inv, !CS, B.gamma / inv, true);
  if (lane == 0) {
    B.inv[j] = inv;
    B.pnorm[j] = nrm;
  }
}

// phase (b) of one feature, ONE thread: the prox's threshold from the running cache (squaredl21.nim:37-43; the rare re-sum
// walks norms in ascending order), the new row's norm and updateCacheBCD (:97-100)
__device__ __forceinline__ void pb_sq_chain(const PbDev& B, int64_t j, double& cache) {
  const double lam = B.gamma / B.inv[j], nrm = B.pnorm[j], old = B.norms[j];
  if (cache < old) {
    double acc = 0.0;
    for (int64_t t = 0; t < B.da; ++t) acc += B.norms[t];
    cache = acc;
  }
  const double lam_scaled = 2.0 * lam / (1.0 + 2 * lam) * (cache - old);
  double factor = 0.0, nn = 0.0;
  if (nrm > lam_scaled) {
    factor = 1.0 - lam_scaled / nrm;
    const double* u = B.row + (size_t)j * B.nc;
    double sq = 0.0;
    for (int s = 0; s < B.nc; ++s) {
      const double x = u[s] * factor;
      sq += x * x;
    }
    nn = sqrt(sq);
  }
  cache -= old;
  B.norms[j] = nn;
  cache += nn;
  B.scale[j] = factor;
}

// ---- OmegaCS: the same schedule and phases, another chain ----
// cache = c, dcache = dc.  dcache is written by initBCD and by prox alone (omegacs.nim:31-35,67-77): it is carried from
// feature to feature, order to order and iteration to iteration of one fit.
struct CsState {
  double c[kCdMaxDeg + 1], dc[kCdMaxDeg + 1];
};

__device__ __forceinline__ void cs_get(CsState& st, const double* g) {
  for (int t = 0; t <= kCdMaxDeg; ++t) {
    st.c[t] = g[t];
    st.dc[t] = g[kCdMaxDeg + 1 + t];
  }
}

__device__ __forceinline__ void cs_put(const CsState& st, double* g) {
  for (int t = 0; t <= kCdMaxDeg; ++t) {
    g[t] = st.c[t];
    g[kCdMaxDeg + 1 + t] = st.dc[t];
  }
}

// one feature's norm into the running polynomials (omegacs.nim:43-44)
__device__ __forceinline__ void cs_push(CsState& st, int deg, double nj) {
  for (int g = 0; g < deg; ++g) st.c[deg - g] += st.c[deg - g - 1] * nj;
}

// recomputeCacheBCD (omegacs.nim:39-45): the polynomials afresh from norms, in ascending j
__device__ __forceinline__ void cs_recompute(const PbDev& B, CsState& st, int deg) {
  for (int t = 0; t <= kCdMaxDeg; ++t) st.c[t] = 0.0;
  st.c[0] = 1.0;
  for (int64_t t = 0; t < B.da; ++t) cs_push(st, deg, B.norms[t]);
}

// min(v) < 0 (omegacs.nim:60,71).  The reference takes the minimum over the whole array, [0 .. the model's degree]; over
// [0 .. deg] it is the same for finite values: cache is zero above deg after every recompute and updateCacheBCD leaves
// those entries alone, and a dcache entry above deg is a lower order's or an earlier step's value, which the check of
// that step (or the recompute it led to, from norms >= 0) left >= 0.
__device__ __forceinline__ bool cs_any_negative(const double* v, int deg) {
  bool neg = false;
  for (int g = 0; g <= deg; ++g) neg = neg || v[g] < 0;
  return neg;
}

// initBCD (omegacs.nim:31-35), once per fit
__global__ void __launch_bounds__(kWave) k_pb_cs_init(PbDev B) {
  const int t = threadIdx.x;
  if (t < 2 * (kCdMaxDeg + 1)) B.chain[t] = t == kCdMaxDeg + 2 ? 1.0 : 0.0;
}

// computeCacheBCD (omegacs.nim:48-51): norms[j] = norm(P[j], 2) a lane per row, then recompute(deg): every lane walks the
// 64 norms in ascending j, one wavefront
__global__ void __launch_bounds__(kWave) k_pb_cs_start(PbDev B) {
  const int lane = threadIdx.x;
  CsState st;
  for (int t = 0; t <= kCdMaxDeg; ++t) st.c[t] = 0.0;
  st.c[0] = 1.0;
  for (int64_t base = 0; base < B.da; base += kWave) {
    const int64_t j = base + lane;
    double nm = 0.0;
    if (j < B.da) {
      double sq = 0.0;
      for (int s = 0; s < B.nc; ++s) {
        const double p = B.at(s, j);
        sq += p * p;
      }
      nm = sqrt(sq);
      B.norms[j] = nm;
    }
    const int cnt = (int)min((int64_t)kWave, B.da - base);
    for (int l = 0; l < cnt; ++l) cs_push(st, B.deg, shfl_d(nm, l));
  }
  if (lane <= kCdMaxDeg) B.chain[lane] = st.c[lane];
}

// phase (b) of one feature, ONE thread: prox from its second step on (omegacs.nim:67-85; the first, the pre-prox row's
// norm, is phase (a)'s), the new row's norm and updateCacheBCD (:54-62).  Both recomputes walk norms in ascending order.
__device__ __forceinline__ void pb_cs_chain(const PbDev& B, int64_t j, CsState& st) {
  const int deg = B.deg;
  const double lam = B.gamma / B.inv[j], nrm = B.pnorm[j];
  double old = B.norms[j];
  for (int g = 2; g <= deg; ++g) st.dc[g] = st.c[g - 1] - st.dc[g - 1] * old;
  if (cs_any_negative(st.dc, deg)) {  // the polynomials without row j, exactly; then the running ones with the pre-prox norm
    B.norms[j] = 0.0;
    cs_recompute(B, st, deg - 1);
    st.dc[0] = 0.0;
    st.dc[1] = 1.0;
    for (int g = 2; g <= deg; ++g) st.dc[g] = st.c[g - 1];
    B.norms[j] = old = nrm;
    cs_recompute(B, st, deg);
  }
  const double thr = lam * st.dc[deg];
  double factor = 0.0, nn = 0.0;
  if (nrm > thr) {
    factor = 1.0 - thr / nrm;
    const double* u = B.row + (size_t)j * B.nc;
    double sq = 0.0;
    for (int s = 0; s < B.nc; ++s) {
      const double x = u[s] * factor;
      sq += x * x;
    }
    nn = sqrt(sq);
  }
  for (int g = 1; g <= deg; ++g) {
    st.c[g] += st.dc[g] * nn;
    st.c[g] -= st.dc[g] * old;
  }
  B.norms[j] = nn;
  if (cs_any_negative(st.c, deg)) cs_recompute(B, st, deg);
  B.scale[j] = factor;
}

// phase (c) of one feature: the new row, delta, viol, the synchronisation
__device__ __forceinline__ void pb_sq_post(const CdDev& D, const PbDev& B, int64_t j, int lane) {
  pb_apply(D, B, j, lane, false, 0.0, B.scale[j]);
  pb_sync(D, B, j, lane);
}

// the chain over features f0 .. f1 (one run) by the calling thread: the running state in registers, written back at the end
template <bool CS>
__device__ __forceinline__ void pb_run_chain(const PbDev& B, int64_t f0, int64_t f1) {
  if constexpr (CS) {
    CsState st;
    cs_get(st, B.chain);
    for (int64_t j = f0; j < f1; ++j) pb_cs_chain(B, j, st);
    cs_put(st, B.chain);
  } else {
    double cache = B.chain[0];
    for (int64_t j = f0; j < f1; ++j) pb_sq_chain(B, j, cache);
    B.chain[0] = cache;
  }
}

template <bool CS>
__global__ void __launch_bounds__(kBlock) k_pb_sq_pre(CdDev D, PbDev B, int64_t f0, int64_t f1) {
  const int64_t j = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (j >= f1) return;
  pb_sq_pre<CS>(D, B, j, threadIdx.x % kWave);
}

template <bool CS>
__global__ void __launch_bounds__(kWave) k_pb_sq_chain(PbDev B, int64_t f0, int64_t f1) {
  if (threadIdx.x != 0) return;
  pb_run_chain<CS>(B, f0, f1);
}

__global__ void __launch_bounds__(kBlock) k_pb_sq_post(CdDev D, PbDev B, int64_t f0, int64_t f1) {
  const int64_t j = f0 + (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (j >= f1) return;
  pb_sq_post(D, B, j, threadIdx.x % kWave);
}

// a sequence of narrow runs r0 .. r1-1, walked by ONE workgroup: (a), a barrier, (b) by thread 0, a barrier, (c), a barrier
template <bool CS>
__global__ void __launch_bounds__(kNarrowBlock) k_pb_sq_runs(CdDev D, PbDev B, int64_t r0, int64_t r1) {
  const int wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t f0 = B.roff[r], f1 = B.roff[r + 1];
    for (int64_t j = f0 + wv; j < f1; j += kNarrowWaves) pb_sq_pre<CS>(D, B, j, lane);
    __syncthreads();
    if (threadIdx.x == 0) pb_run_chain<CS>(B, f0, f1);
    __syncthreads();
    for (int64_t j = f0 + wv; j < f1; j += kNarrowWaves) pb_sq_post(D, B, j, lane);
    __syncthreads();
  }
}

// one dummy feature of fitLower = augment (a column of ones over every sample), one workgroup: the sums over the samples
// are CD's fixed tree, one component after the other; thread 0 takes the step (a chained regulariser continues its running
// state: a dummy feature is a run of one); every thread synchronises its samples.
// CS: OmegaCS, whose two sums over the samples are the reference's own, ascending i (pbcd.nim:130-136): the workgroup forms a
// chunk's terms, thread 0 adds them one after the other.  Its threshold comes from polynomials that cancel
// (dcache[g] = cache[g - 1] - dcache[g - 1] * norms[j]), and with a dummy feature at degree 4 one rounding of these sums
// reaches 1e-10 of P within three iterations; the tree's association is not the reference's.
template <bool CS>
__global__ void __launch_bounds__(kNarrowBlock) k_pb_dummy(CdDev D, PbDev B, int64_t j) {
  __shared__ double red[kNarrowBlock];
  __shared__ double red2[CS ? kNarrowBlock : 1];
  double invsum = 0.0;
  for (int s = 0; s < B.nc; ++s) {
    const double pjs = B.at(s, j);
    double g;
    if constexpr (CS) {
      double iv = 0.0;
      g = 0.0;
      for (int64_t base = 0; base < D.n; base += kNarrowBlock) {
        const int64_t i = base + threadIdx.x;
        double t1 = 0.0, t2 = 0.0;
        if (i < D.n) {
          const double t = pb_derivative(B, D.n, i, s, 1.0, pjs);
          t1 = dloss_at(D, i) * t;
          t2 = t * t;
        }
        red[threadIdx.x] = t1;
        red2[threadIdx.x] = t2;
        __syncthreads();
        if (threadIdx.x == 0) {
          const int cnt = (int)min((int64_t)kNarrowBlock, D.n - base);
          for (int l = 0; l < cnt; ++l) {
            g += red[l];
            iv += red2[l];
          }
        }
        __syncthreads();
      }
      invsum += iv;
    } else {
      double p1 = 0.0, p2 = 0.0;
      for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) {
        const double t = pb_derivative(B, D.n, i, s, 1.0, pjs);
        p1 += dloss_at(D, i) * t;
        p2 += t * t;
      }
      g = block_sum(p1, red);
      invsum += block_sum(p2, red);
    }
    if (threadIdx.x == 0) {
      g /= B.nf;
      g += B.beta * pjs;
      B.row[(size_t)j * B.nc + s] = g;
    }
  }
  if (threadIdx.x == 0) {
    const double inv = pb_inv(D, B, invsum);
    const double lam = B.gamma / inv;
    const bool l1 = !CS && B.reg == NFM_REG_L1, sq = !CS && B.reg == NFM_REG_SQUAREDL21;
    double* u = B.row + (size_t)j * B.nc;
    double acc = 0.0;
    for (int s = 0; s < B.nc; ++s) {
      double x = B.at(s, j) - u[s] / inv;
      if (sq) x /= (1 + 2 * lam);
      u[s] = x;
      acc += x * x;
    }
    const double nrm = sqrt(acc);
    double factor = 1.0;
    if (CS || sq) {
      B.inv[j] = inv;
      B.pnorm[j] = nrm;
      pb_run_chain<CS>(B, j, j + 1);
      factor = B.scale[j];
    } else if (!l1) {
      factor = nrm > lam ? 1.0 - lam / nrm : 0.0;
    }
    double viol = 0.0;
    for (int s = 0; s < B.nc; ++s) {
      const double old = B.at(s, j);
      const double pn = l1 ? soft_threshold(u[s], lam) : (factor == 0.0 ? 0.0 : u[s] * factor);
      B.at(s, j) = pn;
      const double dl = -pn + old;
      B.delta[(size_t)j * B.nc + s] = dl;
      viol += fabs(dl);
    }
    D.out[B.vbase + j] = viol;
  }
  __syncthreads();
  const double* dl = B.delta + (size_t)j * B.nc;
  for (int64_t i = threadIdx.x; i < D.n; i += kNarrowBlock) pb_sync_sample(D, B, dl, i, 1.0);
}

PbDev pb_view(const ModelView& M, int nc, const CdParams& P, CdState* S, int o) {
  PbDev B{};
  B.P = M.P; B.bs = M.bs; B.rs = M.rs; B.Kp = M.Kp; B.kb = M.k; B.kc = M.kc; B.nc = nc;
  B.o = o; B.deg = M.degree - o; B.reg = P.reg;
  B.da = M.da;
  B.vbase = 1 + M.d + (int64_t)o * nc * M.da;
  B.A = S->bA.as<double>(); B.dA = S->bdA.as<double>(); B.row = S->brow.as<double>(); B.delta = S->bdelta.as<double>();
  double* f = S->bfeat.as<double>();
  B.inv = f; B.pnorm = f + M.da; B.scale = f + 2 * M.da; B.norms = f + 3 * M.da;
  B.chain = S->chain.as<double>();
  B.roff = S->roff.as<int64_t>();
  B.beta = P.beta; B.gamma = P.gamma; B.nf = (double)S->n;
  return B;
}

int pb_anova(nfm_ctx* ctx, const CdDev& D, const PbDev& B) {
  hipLaunchKernelGGL(k_pb_anova, dim3(blocks_for(D.n * B.nc, kBlock)), dim3(kBlock), 0, ctx->stream, D, B);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// the run schedule of a chained regulariser over the real features, then the dummy features: a wide run is three launches,
// consecutive narrower ones are walked by one workgroup
template <bool CS>
void pb_runs(hipStream_t st, const CdDev& D, const PbDev& B, CdState* S) {
  const int64_t NR = (int64_t)S->roff_h.size() - 1;
  for (int64_t r = 0; r < NR;) {
    const int64_t f0 = S->roff_h[r], f1 = S->roff_h[r + 1], width = f1 - f0;
    if (width >= kWideMin) {
      const dim3 grid(blocks_for(width, kWavesPerBlock));
      hipLaunchKernelGGL(k_pb_sq_pre<CS>, grid, dim3(kBlock), 0, st, D, B, f0, f1);
      hipLaunchKernelGGL(k_pb_sq_chain<CS>, dim3(1), dim3(kWave), 0, st, B, f0, f1);
      hipLaunchKernelGGL(k_pb_sq_post, grid, dim3(kBlock), 0, st, D, B, f0, f1);
      ++r;
    } else {
      int64_t r1 = r;
      while (r1 < NR && S->roff_h[r1 + 1] - S->roff_h[r1] < kWideMin) ++r1;
      hipLaunchKernelGGL(k_pb_sq_runs<CS>, dim3(1), dim3(kNarrowBlock), 0, st, D, B, r, r1);
      r = r1;
    }
  }
  for (int64_t j = D.d; j < B.da; ++j) hipLaunchKernelGGL(k_pb_dummy<CS>, dim3(1), dim3(kNarrowBlock), 0, st, D, B, j);
}

// epoch (pbcd.nim:160-209) of one order over the real features, then the dummy features
int pb_epoch(nfm_ctx* ctx, const CdDev& D, const PbDev& B, CdState* S) {
  hipStream_t st = ctx->stream;
  if (B.reg == NFM_REG_OMEGACS) {
    hipLaunchKernelGGL(k_pb_cs_start, dim3(1), dim3(kWave), 0, st, B);
    pb_runs<true>(st, D, B, S);
  } else if (B.reg == NFM_REG_SQUAREDL21) {
    hipLaunchKernelGGL(k_pb_norms, dim3(1), dim3(kWave), 0, st, B);
    pb_runs<false>(st, D, B, S);
  } else {
    const int64_t G = (int64_t)S->goff_h.size() - 1;
    const int32_t* order = S->order.as<int32_t>();
    for (int64_t g = 0; g < G;) {
      const int64_t width = S->goff_h[g + 1] - S->goff_h[g];
      if (width >= kWideMin) {
        hipLaunchKernelGGL(k_pb_level, dim3(blocks_for(width, kWavesPerBlock)), dim3(kBlock), 0, st, D, B, order, S->goff_h[g],
                           S->goff_h[g + 1]);
        ++g;
      } else {
        int64_t g1 = g;
        while (g1 < G && S->goff_h[g1 + 1] - S->goff_h[g1] < kWideMin) ++g1;
        hipLaunchKernelGGL(k_pb_levels, dim3(1), dim3(kNarrowBlock), 0, st, D, B, order, S->goff.as<int64_t>(), g, g1);
        g = g1;
      }
    }
    for (int64_t j = D.d; j < B.da; ++j) hipLaunchKernelGGL(k_pb_dummy<false>, dim3(1), dim3(kNarrowBlock), 0, st, D, B, j);
  }
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// a buffer a captured iteration holds the address of
int ensure_held(CdState* S, DevBuf& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return NFM_OK;
  S->drop_graph();
  return b.alloc(bytes);
}

}  // namespace

int pbcd_begin_fit(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int nc, const CdParams& P, CdState* S, const CdDev& D) {
  const size_t cell = sizeof(double) * (size_t)X.n * nc, rows = sizeof(double) * (size_t)std::max<int64_t>(M.da, 1) * nc;
  NFM_TRY(ensure_held(S, S->bA, cell * (M.degree + 1)));
  NFM_TRY(ensure_held(S, S->bdA, cell * M.degree));
  NFM_TRY(ensure_held(S, S->brow, rows));
  NFM_TRY(ensure_held(S, S->bdelta, rows));
  if (!S->bfeat.p || S->bfeat.bytes != sizeof(double) * 4 * std::max<int64_t>(M.da, 1)) {  // pb_view cuts it in four
    S->drop_graph();
    NFM_TRY(S->bfeat.alloc(sizeof(double) * 4 * std::max<int64_t>(M.da, 1)));
  }
  NFM_TRY(ensure_held(S, S->chain, sizeof(double) * 2 * (kCdMaxDeg + 1)));
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_pb_linear, dim3(blocks_for(X.n, kBlock)), dim3(kBlock), 0, st, D);
  if (P.reg == NFM_REG_OMEGACS) hipLaunchKernelGGL(k_pb_cs_init, dim3(1), dim3(kWave), 0, st, pb_view(M, nc, P, S, 0));
  const int no = M.nb / M.kc;
  for (int o = 0; o < no; ++o) {  // with one order this table is carried through the fit (pbcd.nim:292-294)
    const PbDev B = pb_view(M, nc, P, S, o);
    NFM_TRY(pb_anova(ctx, D, B));
    hipLaunchKernelGGL(k_pb_add_top, dim3(blocks_for(X.n, kBlock)), dim3(kBlock), 0, st, D, B);
  }
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

int pbcd_issue_orders(nfm_ctx* ctx, const CsrView& X, const ModelView& M, int nc, const CdParams& P, CdState* S, const CdDev& D) {
  (void)X;
  const int no = M.nb / M.kc;
  for (int o = 0; o < no; ++o) {
    const PbDev B = pb_view(M, nc, P, S, o);
    if (no > 1) NFM_TRY(pb_anova(ctx, D, B));  // rebuilt per order and iteration (pbcd.nim:296-297)
    NFM_TRY(pb_epoch(ctx, D, B, S));
  }
  return NFM_OK;
}

}  // namespace nfm
