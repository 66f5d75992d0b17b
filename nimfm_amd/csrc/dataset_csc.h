// nimfm_amd/csrc/dataset_csc.h -- column-major datasets on the device (dataset_csc.hip): the
// transposition between the two layouts and the row-range filter of a column-major dataset.  Its stacks and normalize are
// dataset_ops.h's routines on the transposed view.
#pragma once
#include "dataset_ops.h"

namespace nfm {

// A compressed matrix seen from its other side (tensor/sparse.nim:490-507 toCSRMatrix, :510-527 toCSCMatrix; one routine,
// the two directions differ in what the caller calls rows).  X: n major segments with minor ids in [0, d).  out: d major
// segments with ids in [0, n); segment j lists the entries of minor id j by ascending major id, and entries of one major
// segment that repeat j keep their storage order.  out->y, has_y are left alone; out->max_row is the longest new segment.
int dsop_transpose(nfm_ctx* ctx, const CsrView& X, DsParts* out);

// X[a..b] of a CSCMatrix (tensor/sparse.nim:300-325).  X: the column arrays as the transposed view (n = nFeatures,
// d = nSamples).  Keeps per column the entries with begin <= id < end, in order, ids rebased by -begin.
int dsop_filter_minor(nfm_ctx* ctx, const CsrView& X, int64_t begin, int64_t end, DsParts* out);

}  // namespace nfm
