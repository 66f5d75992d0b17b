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
// The same CrossSides for a FieldAwareFactorizationMachine (P [F][d][k]) on field-aware sets: U with FU fields, V with FV,
// FU + FV == F ("Invalid nFields."), U.d + V.d == M.d (checked by the caller).  cross[i][j] is decisionFunction
// (model/field_aware_factorization_machine.nim:52-76) of row i of U followed by row j of V with its column ids moved up by
// U.d and its fields by FU (tensor/sparse.nim:719-750).  Every (user entry, item entry) pair has j1 < j2 and counts once:
//   a_u = b + sum_j w_j x_j + sum_{j1 < j2 in u} x1 x2 <P[f2, j1], P[f1, j2]>      c_v = the same of v, shifted, without b
//   A_u[f][g] = sum_{e in u, field(e) = f} x_e P[FU + g, j_e, :]                   B_v[f][g] = sum_{e in v, field(e) = g} x_e P[f, dU + j_e, :]
//   score = (a_u + c_v) + sum_{f, g} <A_u[f][g], B_v[f][g]>
// Both sides are laid out [rows][(f * FV + g) * Kp + s], Kq = FU * FV * Kp rounded up to a multiple of 4, the padding 0.
// FU * FV * Kp > 4096, k > 128, or sides beyond the free memory: NFM_ERR_UNSUPPORTED, naming the pairs and decisionFunction.
int cross_sides_ffm(nfm_ctx* ctx, const CsrView& U, const CsrView& V, const ModelView& M, CrossSides* S);
// out_dev [u_end - u_begin][nV]: the users u_begin .. u_end - 1
int cross_scores(nfm_ctx* ctx, const CrossSides& S, int64_t u_begin, int64_t u_end, double* out_dev);
// ids_dev, scores_dev [nU][K]: per user the K best items by descending score, then ascending id; NaN ranks below every number.
// 1 <= K <= min(nV, kCrossMaxTopK) (checked by the caller).  chunk_items: items per workgroup, 0 = the library's choice;
// rounded up to whole tiles.  The result does not depend on it.
// seen (may be null): [nU x nV], a stored entry (i, j) takes item j out of user i's candidates whatever its value; ranks that
// no candidate fills are ids = -1, scores = NaN.  Without it every rank is filled and nothing of the call changes.
struct AscendingRows {  // the structure of a resident matrix whose rows ascend by column id (repeats allowed)
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
};
int cross_topk(nfm_ctx* ctx, const CrossSides& S, int64_t K, int64_t chunk_items, int64_t* ids_dev, double* scores_dev,
               const AscendingRows* seen = nullptr);
// X's structure as it stands when its rows ascend (the dataset's rows_ascend flag), else with a sorted copy of the ids of
// every row (plan.h: sort_row_ids) held by k0 / k1
int ascending_rows(nfm_ctx* ctx, const CsrView& X, bool rows_ascend, DevBuf* k0, DevBuf* k1, AscendingRows* out);
// out_dev [nnz]: out_dev[e] = cross(U, V)[i][indices[e]] for the entries e of row i, indptr[i] <= e < indptr[i + 1] -- the
// bits cross_scores writes for that pair.  indptr [nU + 1], indices [nnz] < nV: the structure of a resident [nU x nV] matrix.
int cross_pairs(nfm_ctx* ctx, const CrossSides& S, const int64_t* indptr, const int32_t* indices, int64_t nnz, double* out_dev);
// cross_topk over the items stored in the user's row of C [nU x nV] (nnz entries; an id repeated in a row counts once):
// those pairs alone are scored.  Ranks that no candidate fills are ids = -1, scores = NaN.
int cross_topk_among(nfm_ctx* ctx, const CrossSides& S, const AscendingRows& C, int64_t nnz, int64_t K, int64_t* ids_dev, double* scores_dev);
// ranks_dev [nnz]: for the entry e = (i, j) of the held-out structure tptr [nU + 1] / tidx [nnz] (storage order, ids < nV, repeats
// allowed) the number of items j' != j not stored in row i of seen whose (cross[i][j'], j') ranks before (cross[i][j], j) --
// j's place in the full list of user i; -1 where j itself is stored in row i of seen.  n_cand_dev [nU]: nV minus the distinct
// ids of row i of seen (null: every item is a candidate).  chunk_items as for cross_topk; the result does not depend on it.
int cross_rank_of(nfm_ctx* ctx, const CrossSides& S, const int64_t* tptr, const int32_t* tidx, int64_t nnz, const AscendingRows* seen, int64_t chunk_items,
                  int64_t* ranks_dev, int64_t* n_cand_dev);
// precision, recall, ndcg and hit rate at K of the lists ids_dev [nU][K] (-1: an empty rank) against the held-out rows T
// (ascending, distinct ids), each the mean over the users whose row of T is not empty, and their number: out[5], on the host.
// No such user: NaN, NaN, NaN, NaN, 0.
int cross_rank_metrics(nfm_ctx* ctx, int64_t nU, int64_t K, const int64_t* ids_dev, const AscendingRows& T, double out[5]);

}  // namespace nfm
