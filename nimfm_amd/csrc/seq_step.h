// nimfm_amd/csrc/seq_step.h -- what the one-workgroup kernels k_sequential (seq.hip) and k_psgd_seq (psgd_seq.hip) share:
// the reference's per-sample step with thread s on factor s, walking the row IN STORAGE ORDER.
//
// Device: the sample's row behind an accessor (staged in a table once per step, or read from global memory every time), the
// staging of the stored parameter rows, predictWithGrad's forward pass and derivative of one order (optimizer/sgd.nim:146-188)
// and the ascending sum over the factors (sgd.nim:172-173); all inlined, each kernel keeps its barriers and its own `act`.
// Host (at the end): the launch of a one-workgroup kernel and the placement of its per-sample table (LDS, or global memory).
#pragma once
#include "common.h"
#include "fm_device.h"
#include "seq_route.h"

namespace nfm {
namespace seqstep {

// The row in a table (LDS, or global memory: a thread only touches its own column): indices, values and linear weights [mc], the
// stored parameter values [nb][mc][T]; fitLower = augment's dummy features are entries X.d + (q - m) of value 1.  Each kernel lays its own out.
struct StagedRow {
  int64_t* jl;
  double* vl;
  double* wl;
  double* Pl;
  int mc, T, tid;
  __device__ __forceinline__ void sample(int64_t, int) {}
  __device__ __forceinline__ size_t slot(int blk, int q) const { return ((size_t)blk * mc + q) * T + tid; }  // of dA too
  __device__ __forceinline__ int64_t index(int q) const { return jl[q]; }
  __device__ __forceinline__ double value(int q) const { return vl[q]; }
  __device__ __forceinline__ double weight(int q) const { return wl[q]; }
  __device__ __forceinline__ double param(int blk, int q) const { return Pl[slot(blk, q)]; }
  __device__ __forceinline__ double param_at(int blk, int q, size_t) const { return Pl[slot(blk, q)]; }
  __device__ __forceinline__ void set_param(int blk, int q, double v) const { Pl[slot(blk, q)] = v; }
  __device__ __forceinline__ void set_weight(int q, double v) const { wl[q] = v; }

  // indices and values into the table, between the caller's barriers; extra(q, j) is the kernel's own per-entry work
  template <class Extra>
  __device__ __forceinline__ void load_entries(const CsrView& X, int64_t q0, int m, int m_tot, Extra&& extra) const {
    for (int q = tid; q < m_tot; q += T) {
      const int64_t jq = q < m ? (int64_t)X.indices[q0 + q] : X.d + (q - m);
      jl[q] = jq;
      vl[q] = q < m ? X.data[q0 + q] : 1.0;
      extra(q, jq);
    }
  }
  // the stored parameter rows of every block: P[blk][jl[q]][tid] for all q
  __device__ __forceinline__ void load_rows(const ModelView& M, int m_tot) const {
    for (int blk = 0; blk < M.nb; ++blk) {
      int q = 0;
      for (; q + 4 <= m_tot; q += 4) {  // four independent loads in flight
        double t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t4[u] = M.P[M.row(blk, jl[q + u]) * M.Kp + tid];
#pragma unroll
        for (int u = 0; u < 4; ++u) Pl[slot(blk, q + u)] = t4[u];
      }
      for (; q < m_tot; ++q) Pl[slot(blk, q)] = M.P[M.row(blk, jl[q]) * M.Kp + tid];
    }
  }
};

// The row read from global memory wherever it is used (rows too long for the staged layout).
struct GlobalRow {
  const CsrView& X;
  const ModelView& M;
  int64_t q0;  // the sample's first entry and its length: sample()
  int m;
  int mc, T, tid;
  __device__ __forceinline__ void sample(int64_t q0_, int m_) { q0 = q0_, m = m_; }
  __device__ __forceinline__ size_t slot(int blk, int q) const { return ((size_t)blk * mc + q) * T + tid; }
  __device__ __forceinline__ int64_t index(int q) const { return q < m ? (int64_t)X.indices[q0 + q] : X.d + (q - m); }
  __device__ __forceinline__ double value(int q) const { return q < m ? X.data[q0 + q] : 1.0; }
  __device__ __forceinline__ double weight(int q) const { return M.w[X.indices[q0 + q]]; }
  __device__ __forceinline__ double param(int blk, int q) const { return M.P[M.row(blk, 0) * M.Kp + (size_t)index(q) * ((size_t)M.rs * M.Kp) + tid]; }
  __device__ __forceinline__ double param_at(int, int, size_t e) const { return M.P[e]; }  // e = M.row(blk, index(q)) * Kp + tid
  __device__ __forceinline__ void set_param(int, int, double) const {}
  __device__ __forceinline__ void set_weight(int, double) const {}
};

// One order of predictWithGrad for thread tid's factor (seq_anova.inc, the one copy of the recursion) as a function; SCALED:
// the stored values are P / sP (seq.hip's one global scale); PSGD stores the working values: no factor, sP is unused.
// k_psgd_seq calls it.  k_sequential includes the same text in its own body instead: there a function boundary, forced or
// not, changes the register allocation of the whole step (k_sequential<FM, SGD, staged>: 12 more SGPR spill reloads per sample
// and 1.4-1.8 % at 2 entries per row, k = 64, or 52 B of scratch against 44 when forced).  `inline`, not
// __forceinline__: the compiler simplifies the function (A[] becomes registers) before it inlines it; the ISA holds no call.
template <int MAXDEG, bool SCALED, class Row>
__device__ inline double anova_order(const Row& row, int o, int deg, int m_tot, double* dA, double sP = 1.0) {
  double kv = 0.0;
#include "seq_anova.inc"
  return kv;
}

// yh += the sum of the threads' values of block o over s ascending (sgd.nim:172-173), through red[] with a barrier on either
// side.  More than 128 factors: the kc blocks of one order continue ONE ascending sum in tot (kc == 1: tot is the block's sum).
__device__ __forceinline__ void factor_sum(double* red, int tid, int k, double v, int o, int kc, double& tot, double& yh) {
  red[tid] = v;
  __syncthreads();
  if (o % kc == 0) tot = 0.0;
  for (int s = 0; s < k; ++s) tot += red[s];
  if (o % kc == kc - 1) yh += tot;
  __syncthreads();
}

// ---- host: one workgroup of T threads with lds_bytes of dynamic LDS (above 64 KB the kernel's limit is raised first) ----
template <class... KArgs, class... Args>
static int launch_one_workgroup(nfm_ctx* ctx, const char* family, void (*kern)(KArgs...), int T, size_t lds_bytes, const Args&... args) {
  if (lds_bytes > 64 * 1024)
    NFM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  TimedLaunch tl(ctx, family);
  hipLaunchKernelGGL(kern, dim3(1), dim3(T), lds_bytes, ctx->stream, args...);
  NFM_HIP_CHECK(hipGetLastError());
  return NFM_OK;
}

// The per-sample table where seq_sample_table / seq_one_wg_route (seq_route.h) placed it: in LDS (*global = null), else in the
// context's scratch block (its users run in stream order on the context's stream; it grows behind a stream sync).
static int place_sample_table(nfm_ctx* ctx, bool in_lds, size_t table_bytes, double** global) {
  *global = nullptr;
  if (in_lds) return NFM_OK;
  if (!ctx->seq_scratch) ctx->seq_scratch = new DevBuf();
  if (!(ctx->seq_scratch->p && table_bytes <= ctx->seq_scratch->bytes)) {
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    NFM_TRY(ctx->seq_scratch->alloc(table_bytes));
  }
  *global = ctx->seq_scratch->as<double>();
  return NFM_OK;
}

}  // namespace seqstep
}  // namespace nfm
