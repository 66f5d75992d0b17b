// nimfm_amd/csrc/dataset_text.h -- a dataset in HBM -> the bytes of its svmlight / libffm file, formatted on the device
// (dataset_text.hip): dumpSVMLightFile / dumpFFMFile (dataset.nim:793-805, 825-837), and the
// number blocks of the model dump (model/factorization_machine.nim:142-165).
#pragma once
#include "common.h"

namespace nfm {

// where the text goes: a file descriptor, a host buffer of cap bytes, or nowhere (length only)
struct TextSink {
  int fd = -1;
  char* buf = nullptr;
  int64_t cap = 0;
};

// host-side time of a call's steps, for tools/dataset_dump_time.py (the kernels are timed through the context's families
// "dump_len", "dump_scan", "dump_write")
struct TextStats {
  double copy_ms = 0.0, sink_ms = 0.0, total_ms = 0.0;
  int64_t pieces = 0, bytes = 0;
};

// Row i: y_i, then " (j+1):val" (field-aware: " (field+1):(j+1):val") per entry in storage order; "\n" between rows.
// y_host == nullptr: X.y (checked by the caller).  y_int: targets written as integers; one that is not integral or not below
// 2^53 in magnitude is NFM_ERR_INVALID.  chunk_bytes <= 0: the default piece size.  *len_out: the length of the text.
int format_dataset_text(nfm_ctx* ctx, const CsrView& X, const double* y_host, bool y_int, int64_t chunk_bytes, const TextSink& sink,
                        int64_t* len_out, TextStats* stats = nullptr);

// row_len numbers per line separated by one space, every line ended by "\n"; values on the host
int format_f64_text(nfm_ctx* ctx, const double* values, int64_t n_rows, int64_t row_len, char* buf, int64_t cap, int64_t* len_out);

}  // namespace nfm
