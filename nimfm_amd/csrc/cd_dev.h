// nimfm_amd/csrc/cd_dev.h -- what the device code of the column-wise solvers shares: cd.hip (newCD, newPCD; DESIGN.md sections
// 12-13) and pbcd.hip (newPBCD; section 14).
#pragma once
#include "cd.h"
#include "fm_device.h"
#include "prox_dev.h"

namespace nfm {

constexpr int kWideMin = 64;     // a level with at least this many features is a launch of its own (one wavefront each)
constexpr int kNarrowBlock = 1024;  // the one workgroup that walks a run of narrower levels, and the reductions over samples
constexpr int kNarrowWaves = kNarrowBlock / kWave;

struct CdDev {
  const int64_t* rptr;
  const int32_t* ridx;
  const double* rval;
  const int64_t* cptr;
  const int32_t* crow;
  const double* cval;
  const double* y;
  double* yp;
  double* cache;  // [n]: cacheDeg2 (cd.nim:84-88)
  double* A;      // [n][degree + 1]: anova's table (kernels.nim:22-43)
  const double* colsq;
  double* out;    // |update| per coordinate: [intercept | w (d) | P (no x k x (d + nAug))], then the loss sum
  double* w;
  double* sc;
  int64_t n, d;
  int32_t task, loss, A_ld, pad_;
  double lp, mu, a0n, an, bn;
};

// cd.hip's intercept step and w sweep for GreedyCD (gcd.hip), which owns yPred; loss.nim's mu
int cd_issue_intercept(nfm_ctx* ctx, const CdDev& D);
int cd_issue_linear(nfm_ctx* ctx, const CdDev& D, CdState* S);
double cd_loss_mu(int loss);

__device__ __forceinline__ double dloss_at(const CdDev& D, int64_t i) {
  return dev::loss_grad(D.loss, D.lp, dev::target_of(D.y[i], D.task), D.yp[i]);
}

// fixed-tree sum over the kNarrowBlock threads of one workgroup (every thread gets the result)
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kNarrowBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

}  // namespace nfm
