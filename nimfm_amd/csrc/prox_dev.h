// nimfm_amd/csrc/prox_dev.h -- the device code every proximal solver shares: the soft threshold (cd.hip, pbcd.hip, psgd.hip,
// pgd.hip, katyusha.hip), the sum over the lanes of one row and the row-local proximal step (psgd.hip, pgd.hip, katyusha.hip).
//
// The row-local proximal step (NFM_ROW_LOCAL_PROX, at the end) is a macro, not a function, because of a measured codegen
// difference.  As a shared __forceinline__ function -- whole, or the threshold iteration alone, with its inputs by value,
// by reference or through a callable -- the compiler optimises the body before it inlines it (the 2 L + 2 pass loop is
// unrolled out of the kernel's context, branches on kernel arguments are laid out as divergent ones) and the kernels come
// out with another instruction stream: by the signature, +5 to +31 instructions of about 1000 in k_psgd_dense, +91 to +115
// of 773 in k_pgd_trial<1>, +219 to +243 of 1045 in k_pgd_trial<2> and +20 to +281 of 607 to 693 in k_kat_dense; none was
// timed.  The macro expands to the statements the kernels held written out, so every kernel of psgd.o, pgd.o and katyusha.o
// keeps its instruction stream.
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

// The row-local proximal step of the double2 p that lane l of a row's L lanes holds, in place: L1 (l1.nim:35-39), L21
// (l21.nim:23-34), the row norm of SquaredL21 into norm_slot (an lvalue; written by lane 0 of an active row, the coupled
// operator follows in psgd.hip) and the row-wise SquaredL12 (squaredl12.nim:161-162): the vector operator on the row's k
// components by the deterministic threshold iteration of psgd.hip's header.  Every lane of the wavefront runs it: inactive
// rows (act false) keep taking part in the shuffles.  The iteration's break is uniform over the row's lanes; rows of one
// wavefront may differ: a finished row keeps its tau (the map is idempotent at the fixed point).
#define NFM_ROW_LOCAL_PROX(L, reg, reg_transpose, lam, p, act, l, norm_slot)                            \
  do {                                                                                                  \
    if (reg == NFM_REG_L1) {                                                                            \
      p.x = dev::soft_threshold(p.x, lam);                                                              \
      p.y = dev::soft_threshold(p.y, lam);                                                              \
    } else if (reg == NFM_REG_L21 || reg == NFM_REG_SQUAREDL21) {                                       \
      const double nrm = sqrt(dev::row_sum<L>(p.x * p.x + p.y * p.y));                                  \
      if (reg == NFM_REG_L21) {                                                                         \
        const double f = nrm > lam ? 1.0 - lam / nrm : 0.0;                                             \
        p.x = nrm > lam ? p.x * f : 0.0;                                                                \
        p.y = nrm > lam ? p.y * f : 0.0;                                                                \
      } else if (act && l == 0) {                                                                       \
        norm_slot = nrm;                                                                                \
      }                                                                                                 \
    } else if (reg == NFM_REG_SQUAREDL12 && !reg_transpose) {                                           \
      const double ax = fabs(p.x), ay = fabs(p.y);                                                      \
      double tau = 0.0;                                                                                 \
      int cnt_prev = -1;                                                                                \
      for (int pass = 0; pass < 2 * L + 2; ++pass) {                                                    \
        const double S = dev::row_sum<L>((ax > tau ? ax : 0.0) + (ay > tau ? ay : 0.0));                \
        const int c = (int)dev::row_sum<L>((double)((ax > tau) + (ay > tau)));                          \
        if (c == cnt_prev || c == 0) break;                                                             \
        cnt_prev = c;                                                                                   \
        tau = 2 * lam * (S / (1.0 + 2.0 * lam * (double)c));                                            \
      }                                                                                                 \
      p.x = dev::soft_threshold(p.x, tau);                                                              \
      p.y = dev::soft_threshold(p.y, tau);                                                              \
    }                                                                                                   \
  } while (0)
