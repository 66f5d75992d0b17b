// nimfm_amd/csrc/model_text.h -- the number blocks of a model dump, text -> float64, parsed on the device (model_text.hip,
// DESIGN.md section 31): the way back in of format_f64_text (dataset_text.h).  The blocks are those `load` reads
// (model/factorization_machine.nim:168-220, field_aware_factorization_machine.nim:119-158,
// convex_factorization_machine.nim:111-164).
#pragma once
#include "common.h"
#include "dataset_text.h"  // TextStats

namespace nfm {

// The first n_rows lines of text[0, len) (host memory), row_len numbers each -> values[row * row_len + col] (host).
// chunk_bytes <= 0: pieces of 128 MiB.  *consumed: the bytes through the n_rows-th '\n' (len when the last line has none).
// *clean = 0: the text is not in that form (model_text_pieces.h) and values is unspecified.  stats: pieces walked, bytes of
// text, the uploads and copies back (HIP events) in copy_ms, the staging memcpy in sink_ms, the whole call in total_ms.
int parse_f64_text(nfm_ctx* ctx, const char* text, int64_t len, int64_t n_rows, int64_t row_len, int64_t chunk_bytes, double* values,
                   int64_t* consumed, int32_t* clean, TextStats* stats = nullptr);

}  // namespace nfm
