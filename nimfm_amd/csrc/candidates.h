// nimfm_amd/csrc/candidates.h -- sampleCandidates: per user a uniform sample of the items that a resident [nU x nV] matrix
// does not store, as a new resident matrix whose stored entries are the candidates (candidates.hip).
// The reference has no counterpart: it scores the rows it is given (model/factorization_machine.nim:100-122).
//
// For user i, with wrapping uint64 arithmetic:
//   X_i      the ascending distinct ids of row i of exclude or of include;  E_i = nV - |X_i|;  n_i = min(nPerUser, E_i)
//   elig(r)  the r-th non-negative integer not in X_i: r + p, p the smallest index with X_i[p] - p > r (|X_i|: none)
//   draw(t)  mulhi64(mix(seed + 0x9E3779B97F4A7C15 (i 2^32 + t + 1)), E_i), mix = splitmix64's finaliser
//   first(m) the first m distinct values of draw(0), draw(1), ...
//   S_i      n_i == E_i: every eligible item;  n_i <= E_i / 2: elig(first(n_i));  else: every eligible item but
//            elig(first(E_i - n_i))
// Row i of the result: the ascending union of S_i and the ids of row i of include, values 1.0.  A pure function of
// (exclude, include, nPerUser, seed): no grid, chunk or storage order enters it.
#pragma once
#include "cross.h"
#include "dataset_ops.h"

namespace nfm {

// the most candidates drawn per user: the sorted list of one user's draws is one wavefront's kCandMax int32 of LDS
// (tests/test_gpu_candidates.py reads the number from this file)
constexpr int kCandMax = 1024;

__host__ __device__ inline uint64_t cand_mix(uint64_t seed, uint64_t i, uint64_t t) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((i << 32) + t + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// exclude, include (may be null): the structures of two resident [nU x nV] matrices, rows ascending (ascending_rows), repeats
// allowed; 1 <= n_per_user <= kCandMax and nV <= 2^31 - 1 - 64 (checked by the caller).  out: the arrays of the result.
int sample_candidates(nfm_ctx* ctx, const AscendingRows& exclude, int64_t exclude_nnz, const AscendingRows* include, int64_t include_nnz, int64_t nU,
                      int64_t nV, int64_t n_per_user, uint64_t seed, DsParts* out);

}  // namespace nfm
