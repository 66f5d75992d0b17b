// nimfm_amd/csrc/psgd_seq.h -- PSGD (optimizer/psgd.nim): SGD in the reference's sample order with the lazily caught-up
// sparsity regularisers L1 and L21 (regularizer/l1.nim, l21.nim).  Kernels and launch loop: psgd_seq.hip.
// (psgd.hip / OPT_PSGD are MBPSGD, the mini-batch solver.)
#pragma once
#include "opt_views.h"

namespace nfm {

// what the persistent kernel leaves in ctl[1] when it stops early: the dense pass that is due before the next sample
enum { PSGD_DUE_W = 1 /* psgd.nim:162-166 */, PSGD_DUE_CACHE = 2 /* resetCacheSGD, l1.nim:113-126 / l21.nim:90-101 */ };
// the scalar block: the regulariser's scaling and threshold, psgd.nim's scaling_w, the running loss of the current call
enum { PS_SCALING = 0, PS_THRESHOLD = 1, PS_SCALING_W = 2, PS_LOSS = 3, PS_COUNT = 8 };

struct PsgdSeqView {
  double* scalings;    // [d + nAug]  reg.scalings (one pair of snapshot arrays serves all orders, l1.nim:47-52)
  double* thresholds;  // [d + nAug]  reg.thresholds
  double* scalings_w;  // [d]         psgd.nim:98
  double* sc;          // [PS_COUNT]
  int64_t* ctl;        // [2] position of the next sample, PSGD_DUE_* mask
};

struct PsgdSeqState {  // kept on the optimizer handle
  DevBuf arena;  // [scalings | thresholds | scalings_w | sc | ctl]
  PsgdSeqView v{};
  int64_t d = 0, da = 0;
  bool fit_ready = false;  // nfm_psgd_begin_fit ran on (fit_uid, fit_serial)
  uint64_t fit_uid = 0, fit_serial = 0;
  int64_t cache_resets = 0, w_resets = 0;  // dense passes since begin_fit
};

// the half-open pieces a range [begin, end) is run in: the persistent kernel stops after the sample that makes a dense
// pass due and reports the position it reached; the loop runs the pass and relaunches from there.  Plain bookkeeping, no
// device code: next position and mask in, what to launch next out.
struct PsgdSeqCursor {
  int64_t pos, end, it0, begin;
  PsgdSeqCursor(int64_t b, int64_t e, int64_t it) : pos(b), end(e), it0(it), begin(b) {}
  bool done() const { return pos >= end; }
  int64_t it() const { return it0 + (pos - begin); }  // the step counter of the sample at pos
  // the kernel reported (next, due): false when the report is not a position inside (pos, end]
  bool advance(int64_t next, int64_t due) {
    if (next <= pos || next > end || (due & ~(int64_t)(PSGD_DUE_W | PSGD_DUE_CACHE))) return false;
    if (!due && next != end) return false;  // it may stop early only for a dense pass
    pos = next;
    return true;
  }
};

int psgd_seq_alloc(nfm_ctx* ctx, const ModelView& M, PsgdSeqState* S);
// initSGD (l1.nim:47-52, l21.nim:38-43) and psgd.nim:97-98: every cache back to its start
int psgd_seq_begin_fit(nfm_ctx* ctx, const ModelView& M, PsgdSeqState* S);
// psgd.nim:122-184 over perm[begin .. end) (perm_dev indexed by absolute position, or null); *loss_sum = the running loss of the range
int psgd_seq_run(nfm_ctx* ctx, const CsrView& X, const ModelView& M, const OptView& O, PsgdSeqState* S, const int64_t* perm_dev, int64_t begin,
                 int64_t end, int64_t it0, int m_cap, double* loss_sum);
// finalize (psgd.nim:58-73): the w catch-up, then lazyUpdateFinal
int psgd_seq_finalize(nfm_ctx* ctx, const ModelView& M, const OptView& O, PsgdSeqState* S);

}  // namespace nfm
