// nimfm_amd/csrc/dataset_stream.h -- a compressed matrix in HBM -> the bytes of the reference's binary stream file
// (tensor/sparse_stream.nim:3-33), packed on the device (dataset_stream.hip): the writer of
// STREAMCSR / STREAMCSRFIELD / STREAMCSC files for nfm_dataset_dump_stream, nfm_transpose_file, nfm_convert_ffm and
// nfm_convert_svmlight.
#pragma once
#include "common.h"
#include "dataset_text.h"  // TextSink, TextStats

namespace nfm {

enum { STREAM_CSR = 0, STREAM_CSRFIELD = 1, STREAM_CSC = 2 };
constexpr int kStreamHeadMax = 14 + 48;

// max / min of the header as the reference folds them (dataset.nim:1021-1022, 1052-1053): from -Inf / +Inf,
// max(maxVal, val) / min(minVal, val) over the values in storage order -- a NaN never replaces the bound, and of values that
// compare equal (+0.0 / -0.0) the first in storage order stays.
int stream_minmax(nfm_ctx* ctx, const double* data, int64_t nnz, double* vmax, double* vmin);

// magic and header {nRows, nCols, nnz[, nFields], max, min} -> head (kStreamHeadMax bytes of room); returns their length:
// 49 bytes, 62 for STREAM_CSRFIELD
int stream_head(int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_fields, double vmax, double vmin, char* head);

// head[0, head_len), then per record r < X.n an int64 count and count x {val: f64, id: i64} (X.fields: {field: i64, val, id}):
// id = X.indices + id_add, field = X.fields + field_add.  X is a view of either orientation (a column-major dataset passes
// its column arrays).  chunk_bytes <= 0: the default piece size.  A sink that goes nowhere: the length only.
int pack_stream(nfm_ctx* ctx, const CsrView& X, int64_t id_add, int64_t field_add, const char* head, int head_len, int64_t chunk_bytes,
                const TextSink& sink, int64_t* len_out, TextStats* stats = nullptr);

}  // namespace nfm
