// nimfm_amd/csrc/dataset_ops.h -- datasets made from datasets on the device (dataset_ops.hip):
// row selection and slices, vstack / hstack, normalize, and the user-item-rating text loader.
#pragma once
#include "common.h"

namespace nfm {

// the arrays of a dataset under construction; api.hip turns them into a nfm_dataset (uid, repeats, views)
struct DsParts {
  DevBuf indptr, indices, data, fields, y;  // int64[n+1], int32[nnz], double[nnz], int32[nnz]?, double[n]?
  int64_t n = 0, d = 0, nnz = 0, n_fields = 0;
  bool has_fields = false, has_y = false;
  int max_row = 0;
  int64_t bytes = 0;  // the rating loader's text, upload and parse time
  double upload_ms = 0.0, parse_ms = 0.0;
};

enum { NORM_L1 = 0, NORM_L2 = 1, NORM_LINFTY = 2 };  // NormKind, tensor/sparse.nim:37-38

// X[rows] (tensor/sparse.nim:263-285, 333-357).  rows_host == nullptr: the slice [begin, begin + m).  The ids are checked
// by the caller.
int dsop_select_rows(nfm_ctx* ctx, const CsrView& X, const int64_t* rows_host, int64_t begin, int64_t m, DsParts* out);
// tensor/sparse.nim:564-581, 613-633 / :671-698, 719-750.  Shapes and kinds are checked by the caller.
int dsop_vstack(nfm_ctx* ctx, const CsrView* parts, int n_parts, DsParts* out);
int dsop_hstack(nfm_ctx* ctx, const CsrView* parts, int n_parts, DsParts* out);
// tensor/sparse.nim:372-411 into a copy
int dsop_normalize(nfm_ctx* ctx, const CsrView& X, int axis, int norm, DsParts* out);
// loadUserItemRatingFile (dataset.nim:840-900); path != nullptr: the file, else mem[0, mem_len)
int dsop_user_item(nfm_ctx* ctx, const char* path, const char* mem, int64_t mem_len, DsParts* out);

}  // namespace nfm
