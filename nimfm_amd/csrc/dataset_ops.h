// nimfm_amd/csrc/dataset_ops.h -- datasets made from datasets on the device (dataset_ops.hip):
// row selection and slices, vstack / hstack, normalize, and the user-item-rating text loader.
//
// Every routine here works on (major pointer, minor ids, values): a CsrView whose n counts the MAJOR segments and whose d
// bounds the minor ids.  A row-major dataset passes itself; a column-major one (dataset_csc.h) passes
// its column arrays as the view of the transposed matrix (n = nFeatures, d = nSamples, y = nullptr), so CSC hstack IS
// dsop_vstack, CSC vstack IS dsop_hstack (the id offset of a part is the view's d) and CSC normalize(axis) IS
// dsop_normalize(1 - axis) -- the same device code for both layouts.
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
// loadUserItemRatingFile (dataset.nim:840-900); path != nullptr: the file, else mem[0, mem_len).  short_lines: lines of
// fewer than 5 characters are skipped, as the loader of a column-major dataset skips them (dataset.nim:923, 955, 975)
int dsop_user_item(nfm_ctx* ctx, const char* path, const char* mem, int64_t mem_len, DsParts* out, bool short_lines = false);

// ---- what dataset_csc.hip shares with dataset_ops.hip ----
// the launch geometry of every dataset kernel: at most n_cu * 8 workgroups of kBlock threads, `per` items per workgroup
inline unsigned dsop_grid(const nfm_ctx* ctx, int64_t n, int per = kBlock) {
  int64_t b = (n + per - 1) / per;
  const int64_t cap = (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}
// out[i] = in[0] + ... + in[i - 1] for i < count (hipcub; synchronizes the stream)
int dsop_exclusive_scan(hipStream_t st, const int64_t* in, int64_t* out, int64_t count);
// a copy kernel in the widest words both pointers allow
int dsop_copy(nfm_ctx* ctx, void* dst, const void* src, size_t bytes);
// room for the entry arrays (at least one element each)
int dsop_alloc_entries(DsParts* out, int64_t nnz, bool with_fields);

}  // namespace nfm
