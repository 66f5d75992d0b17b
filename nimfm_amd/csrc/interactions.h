// nimfm_amd/csrc/interactions.h -- which feature interactions a fitted factorization machine uses (interactions.hip, DESIGN.md
// section 36).  The reference's sparse-FM benchmarks end with three numbers of the interaction matrix of one order
// (benchmarks/ml100k/utils.nim: countInteractions, countFeatures; norm(matmul(P.T, P), 1)):
//   W = Q diag(lams) Q^T,   Q[j][s] = P[order][s][j],   j < da = d + nAugments
// W is never stored: the rows of Q that are not all zero are compacted (ascending by id), W is formed tile by tile on the f64
// matrix instruction and reduced where it is made -- sum |W_ij|, the pairs i < j with W_ij != 0, the features that are in one --
// or its K largest entries are kept.  A tile whose rows and columns share no factor is skipped on a 64-bit signature.
//
// Arithmetic: W_ij is the matrix unit's chain (fused, the factors ascending four at a time, lams applied to the column
// operand), as crossDecisionFunction's product is: a pair whose non-zero terms cancel exactly in the reference's unfused sum may
// differ from it in the last place and so in "!= 0".  A pair with no factor in which both rows are non-zero is exactly +0 for
// finite parameters, in any arithmetic, and is never counted or ranked.
#pragma once
#include "common.h"

namespace nfm {

// The tile: a workgroup of kBlock lanes owns kInterT x kInterT entries of W (rows and columns of the same compacted matrix) and
// walks the factors in steps of kInterKS.  (tests/test_gpu_interactions.py reads the numbers from this file.)
constexpr int kInterT = 64;
constexpr int kInterKS = 32;
constexpr int kInterMaxTopK = 256;
constexpr int kInterGridPerCU = 4;  // workgroups per CU of the tile walk: a launch's grid is at most n_cu * kInterGridPerCU

struct InterRows {
  DevBuf Qc;    // [dn][Kq] the rows of Q that are not all zero, scale applied; Kq = kc * Kp rounded up to a multiple of 4, padding 0
  DevBuf ids;   // [dn] int64: the feature of a kept row, ascending
  DevBuf sig;   // [dn] uint64: bit s & 63 for every non-zero Q[j][s]
  DevBuf tsig;  // [ceil(dn / kInterT)] uint64: the OR over a tile's rows
  const double* lams = nullptr;  // the order's [kc * Kp] weights (the model's own array)
  int64_t dn = 0;
  int Kq = 0, nlam = 0;
};

// M: a FactorizationMachine (not field-aware, not convex: checked by the caller), 0 <= order < nOrders.
int inter_rows(nfm_ctx* ctx, const ModelView& M, int order, InterRows* R);
// out_l1[2]: sum |W_ij| over all i, j; over i != j.  out_counts[3]: pairs i < j with W_ij != 0 (-0 is zero, NaN is not), features
// in such a pair, rows of Q that are not all zero.  The per-tile sums are folded in one fixed order: the same bits every run.
int inter_stats(nfm_ctx* ctx, const InterRows& R, double* out_l1, int64_t* out_counts);
// pairs [K][2], weights [K], on the host: the pairs i < j with W_ij != 0 by descending |W_ij|, then ascending i, then ascending
// j, the weight signed; NaN ranks below every number; ranks that no pair fills: -1, -1, NaN.  1 <= K <= kInterMaxTopK.
int inter_topk(nfm_ctx* ctx, const InterRows& R, int64_t K, int64_t* pairs, double* weights);

}  // namespace nfm
