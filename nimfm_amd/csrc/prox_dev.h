// nimfm_amd/csrc/prox_dev.h -- the device code every proximal solver shares: the soft threshold (cd.hip, pbcd.hip, psgd.hip,
// pgd.hip) and the sum over the lanes of one row (psgd.hip, pgd.hip).
//
// The row-local proximal step itself (L1, L21, the SquaredL21 norms, the row-wise SquaredL12 threshold iteration) stays
// written out in k_psgd_dense and k_pgd_trial.  As a shared __forceinline__ function -- whole, or the threshold iteration
// alone, with its inputs by value, by reference or through a callable -- the compiler optimises the body before it inlines
// it (the 2 L + 2 pass loop is unrolled out of the kernel's context, branches on kernel arguments are laid out as divergent
// ones) and both kernels come out with another instruction stream: by the signature, +5 to +31 instructions of about 1000 in
// k_psgd_dense, +91 to +115 of 773 in k_pgd_trial<1> and +219 to +243 of 1045 in k_pgd_trial<2>; none was timed.  Sharing it is open: it wants that
// measurement first.  Until then tests/test_prox_copies.py holds the two texts to each other.
#pragma once
#include "fm_device.h"

namespace nfm {
namespace dev {

// softthreshold (regularizer/utils.nim:4-5): float64(sgn(x)) * max(abs(x) - alpha, 0.0).  0.0 * t keeps the reference's
// NaN at x == 0 with an infinite t.
__device__ __forceinline__ double soft_threshold(double x, double alpha) {
  const double t = fmax(fabs(x) - alpha, 0.0);
  return x > 0 ? t : (x < 0 ? -t : 0.0 * t);
}

// sum over the L lanes of one row (fixed xor tree; every lane of the row ends with the same bits)
template <int L>
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
  for (int s = 1; s < L; s <<= 1) v += shfl_xor_d(v, s);
  return v;
}

}  // namespace dev
}  // namespace nfm
