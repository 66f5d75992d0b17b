// nimfm_amd/csrc/extmath.h -- sparse x dense products of resident datasets (extmath.hip):
// matmul(S, D), matmul(D, S), mvmul(S, vec), vmmul(vec, S) of extmath.nim:10-133.
//
// One kernel family, "sparse segment times dense rows": a CsrView whose n counts the MAJOR segments (dataset_ops.h) and a
// dense matrix whose rows are indexed by the view's minor ids.  The row structure of S serves S . D and mvmul, its column
// structure (as the view of the transposed matrix) D . S and vmmul.
#pragma once
#include "common.h"

namespace nfm {

constexpr int kSpmmAcc = 4;      // double2 accumulators a lane holds: a column panel is up to 64 * kSpmmAcc 16-byte words
constexpr int kSpmmUnroll = 4;   // entries whose dense rows are in flight per lane
constexpr int kSpmmStage = 256;  // entries of a wavefront's staging buffer in LDS: one coalesced 48-byte read per lane
constexpr int kSpmmPanel = kWave * kSpmmAcc * 2;  // dense columns of one panel at 64 lanes per segment

// lanes per segment for r dense columns: the power of two that covers the row's 16-byte words, at most a wavefront.  A
// function of r alone, so the chain of an output element does not depend on the matrix its segment stands in.
inline int spmm_team(int64_t r) {
  const int64_t words = (r + 1) / 2;
  int T = 1;
  while (T < kWave && T < words) T <<= 1;
  return T;
}

// R[i][c] = sum over the entries (j, val) of segment i of X, in storage order, of val * D[j][c], from +0.0, every product and
// every sum rounded by itself.  D [X.d x r] and R [X.n x r] are row-major device arrays of any alignment.  Enqueued on the
// context's stream; nothing is synchronized.
int launch_spmm(nfm_ctx* ctx, const CsrView& X, const double* D, int64_t r, double* R);

// out [cols x rows] = in [rows x cols] transposed, both row-major device arrays; enqueued on the context's stream
int launch_transpose_f64(nfm_ctx* ctx, const double* in, int64_t rows, int64_t cols, double* out);

}  // namespace nfm
