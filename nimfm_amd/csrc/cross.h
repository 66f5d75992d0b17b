// nimfm_amd/csrc/cross.h -- every pair of two row sets scored by a degree-2 factorization machine, and the K best items of
// every user (cross.hip).  cross(U, V)[i][j] is decisionFunction (model/factorization_machine.nim:100-122,
// kernels.nim:59-64) of row i of U followed by row j of V with its column ids moved up by U's width (tensor/sparse.nim:671-698).
//
// With q_s(x) = sum_j P[s,j] x_j and r_s(x) = sum_j (P[s,j] x_j)^2 the joined row factorises:
//   f(u + v) = [b + lin(u) + 1/2 sum_s lam_s (q_s(u)^2 - r_s(u))] + [lin(v) + 1/2 sum_s lam_s (q_s(v)^2 - r_s(v))]
//              + sum_s (lam_s q_s(u)) q_s(v)
// -- two passes of the size of decisionFunction(U) and decisionFunction(V) (k_cross_side) and one [nU x Kq] . [Kq x nV]
// product (cross_tile: the f64 matrix instruction).
#pragma once
#include "common.h"

namespace nfm {

// The tile of the product: a workgroup of kBlock lanes owns kCrossTU users x kCrossTV items and walks the factors in steps
// of kCrossKS.  (tests/test_gpu_cross.py reads the three numbers from this file.)
constexpr int kCrossTU = 32;
constexpr int kCrossTV = 64;
constexpr int kCrossKS = 32;
constexpr int kCrossMaxTopK = 256;

struct CrossSides {
  DevBuf qU, qV;  // [nU][Kq] lam_s q_s(u), [nV][Kq] q_s(v); Kq = the model's kc * Kp factors, a multiple of 4, padding 0
  DevBuf aU, cV;  // [nU] b + lin(u) + 1/2 sum_s lam_s (q_s^2 - r_s), [nV] the same of v without b
  int64_t nU = 0, nV = 0;
  int Kq = 0;
};

// U.d + V.d == M.d, M a degree-2 FM of one order (checked by the caller).  The dummy feature of fitLower = augment joins U.
int cross_sides(nfm_ctx* ctx, const CsrView& U, const CsrView& V, const ModelView& M, CrossSides* S);
// out_dev [u_end - u_begin][nV]: the users u_begin .. u_end - 1
int cross_scores(nfm_ctx* ctx, const CrossSides& S, int64_t u_begin, int64_t u_end, double* out_dev);
// ids_dev, scores_dev [nU][K]: per user the K best items by descending score, then ascending id; NaN ranks below every number.
// 1 <= K <= min(nV, kCrossMaxTopK) (checked by the caller).  chunk_items: items per workgroup, 0 = the library's choice;
// rounded up to whole tiles.  The result does not depend on it.
int cross_topk(nfm_ctx* ctx, const CrossSides& S, int64_t K, int64_t chunk_items, int64_t* ids_dev, double* scores_dev);

}  // namespace nfm
