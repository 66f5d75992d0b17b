// nimfm_amd/csrc/mb_dev.h -- what the two mini-batch drivers share on the device: the records the row phase leaves for the column
// phase, the size of the decay-correction table, and the kernels of mb_fm.hip that mb_ffm.hip launches as well.  Included by
// mb_fm_kernels.h (FactorizationMachine) and mb_ffm.hip (FieldAwareFactorizationMachine).
#pragma once
#include "opt_views.h"

namespace nfm {

struct SampleRec {
  double dL, etaP, etaw, yhat;  // yhat: the sample's prediction (read back by predictAllWithGrad; the field-aware row phase stores 0)
};
struct PartA {
  double loss, viol, acc0, acc1;
};

static_assert(sizeof(SampleRec) == 32 && sizeof(PartA) == 32, "record layout");

constexpr int kFtab = 64;  // touch counts 1..kFtab have a tabulated decay correction: k_schedule writes Ftab, both column phases read it

// defined once, in mb_fm.hip
// per-batch decay products Dtab [nb][4] and decay corrections by touch count Ftab [nb][2][kFtab] (SGD)
__global__ void k_schedule(OptView O, int fit_linear, int fit_intercept, const int64_t* __restrict__ bat_pos,
                           const double* __restrict__ it0p, double* __restrict__ Dtab, double* __restrict__ Ftab);
// the scales at every batch boundary Stab [nb + 1][2]
__global__ void k_scale_prefix(double* __restrict__ sc, const double* __restrict__ Dtab, double* __restrict__ Stab, int64_t nb);
// adds the last batch's per-block viol partials (every other batch's are folded in by the next batch's closing workgroup)
__global__ void k_epoch_close(const double* __restrict__ parts, int n, double* __restrict__ out_acc);
__global__ void k_set_double(double* p, double v);

}  // namespace nfm
