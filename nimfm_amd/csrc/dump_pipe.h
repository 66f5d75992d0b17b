// nimfm_amd/csrc/dump_pipe.h -- the way out of the device for a file made there piece by piece (DESIGN.md sections 24, 30):
// two device buffers, the process's two pinned host buffers and a copy stream.  The copy to the host and the write() of
// piece p run beside the making of piece p + 1.  dataset_text.hip (text) and dataset_stream.hip (the binary stream format)
// are its users; the definitions are in dataset_text.hip.
#pragma once
#include <mutex>

#include "dataset_text.h"

namespace nfm {

double dump_now_ms();  // a steady host clock, in milliseconds

struct DumpPipe {
  std::unique_lock<std::mutex> pinned_lock;  // first member: released after everything below has been given back
  nfm_ctx* ctx = nullptr;
  hipStream_t copy_stream = nullptr;
  struct Slot {
    DevBuf out;              // the piece on the device, out_cap bytes (16-byte aligned)
    char* pin = nullptr;     // one of the pinned pair
    int64_t* tot = nullptr;  // pinned: four words the maker of a piece may copy its totals into
    hipEvent_t fmt = nullptr, c0 = nullptr, c1 = nullptr;
    int64_t len = 0;
    bool busy = false;
  } slot[2];
  TextSink sink;
  int64_t written = 0;  // bytes handed to the sink so far
  double copy_ms = 0.0, sink_ms = 0.0;

  // length_only: no buffers, no copy stream -- the slots' totals and `fmt` events only
  int open(nfm_ctx* ctx, const TextSink& sink, int64_t out_cap, bool length_only);
  // len bytes from the host straight to the sink (a file's header)
  int put(const char* p, int64_t len);
  // piece S.len of S.out is complete on the context's stream (the caller has waited for S.fmt): queue its copy out
  int send(Slot& S);
  // the piece's copy has been queued: wait for it, hand the bytes on.  Nothing to do for a slot that is not busy.
  int consume(Slot& S);
  // both streams are drained before the device blocks go back to the cache and the pinned pair is released
  ~DumpPipe();
};

}  // namespace nfm
