// nimfm_amd/csrc/api.hip -- the C ABI of include/nimfm_hip.h over the HIP kernels.
// Host-side bookkeeping only (allocation, layout conversion launches, plan cache, epoch driver);
// every entry point validates shapes on the host before any kernel is launched.
#include <fcntl.h>
#include <math.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "cd.h"
#include "cfm.h"
#include "cross.h"
#include "dataset_csc.h"
#include "dataset_ops.h"
#include "dataset_stream.h"
#include "dataset_text.h"
#include "gcd.h"
#include "psgd_seq.h"
#include "dp.h"
#include "dump_pipe.h"
#include "ingest.h"
#include "mb.h"
#include "katyusha.h"
#include "model_text.h"
#include "pgd.h"

using namespace nfm;

struct nfm_dataset {
  nfm_ctx* ctx = nullptr;
  CsrView v{};
  DevBuf indptr, indices, data, fields, y;
  bool has_y = false;
  int max_row = 0;
  int64_t repeats = 0, repeat_row = -1;  // entries that repeat a column id of their row (plan.h: predict-only data)
  bool rows_ascend = true;  // every row's column ids ascend in storage order (established with `repeats`, by the same pass)
  int64_t ingest_bytes = 0;  // set by the text loaders (ingest.hip)
  double ingest_upload_ms = 0.0, ingest_parse_ms = 0.0;
  // Cache keys.  uid: process-unique, never reused -- what a Plan is keyed by (a raw nfm_dataset* can be handed out
  // again by `new` after a `delete`, for a dataset of the same shape and different structure).  serial: bumps whenever
  // one of the v.* device pointers changes (nfm_dataset_set_targets) -- a captured hipGraph holds those pointers.
  uint64_t uid = 0, serial = 0;
  uint64_t y_gen = 0;  // bumps with every nfm_dataset_set_targets: what a fit's target-dependent state (pgd.h) was begun on
  CscIndex csc;  // column-major twin, built by the first plan that can use it (plan.hip)
  std::unique_ptr<Plan> diag_plan;  // the plan nfm_dataset_plan_build made for reading back; no optimizer sees it
  // NFM_LAYOUT_CSC: the dataset IS the column arrays below; everything above then describes its row
  // twin (toCSRMatrix of the columns, made with the dataset), which is what every consumer of rows runs on unchanged
  int layout = NFM_LAYOUT_CSR;
  DevBuf c_indptr, c_indices, c_data;  // int64[nFeatures + 1], int32[nnz] sample ids, double[nnz]
  CsrView cv{};  // the column arrays as the view of the transposed matrix: n = nFeatures, d = nSamples, y = nullptr
};
// what a consumer of rows in storage order says to a column-major dataset (the reference rejects it at compile time)
static int refuse_csc(const nfm_dataset* ds, const char* what) {
  NFM_CHECK(ds->layout != NFM_LAYOUT_CSC, NFM_ERR_UNSUPPORTED,
            "%s takes a row-major dataset, not a CSCDataset: convert it with toCSRDataset (nfm_dataset_to_csr)", what);
  return NFM_OK;
}
static uint64_t next_dataset_uid() {
  static std::atomic<uint64_t> g{0};
  return ++g;
}

struct Span {  // a piece of an arena allocation
  void* p = nullptr;
  size_t bytes = 0;
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};
static size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

struct nfm_model {
  uint64_t uid = 0;  // process-unique; optimizers refer to their model by it (an address can be handed out again)
  nfm_ctx* ctx = nullptr;
  nfm_model_cfg cfg{};
  // k: n_components; FMs with k > 128: the factors of an order are cut into kc device blocks of kb <= 128 factors
  // (ModelView::kc) -- nb counts DEVICE blocks (orders x kc; fields for field-aware models), no the reference's orders
  int nb = 0, no = 0, kc = 1, kb = 0, n_aug = 0, k = 0, Kp = 0, L = 0;
  int64_t d = 0, da = 0;
  // a wide FM of ONE order keeps its kc blocks FEATURE-major: the row of a feature is one contiguous run of kc * Kp doubles -- kc
  // blocks of Kp to the kernels that walk blocks (row(b, j) = j * kc + b), ONE row of kc * Kp factors to the one-sample-in-flight
  // kernel (seq_row_view: its pipelined step and its single ascending factor sum, as before round 5), blocks of 64 to the window
  // (seq_window_view).  Several orders: order-major blocks (the views above need one stride per block).
  bool wide_rows() const { return cfg.kind == NFM_KIND_FM && kc > 1 && no == 1; }
  int64_t bs_() const { return (cfg.kind == NFM_KIND_FFM || wide_rows()) ? 1 : da; }
  int64_t rs_() const { return (cfg.kind == NFM_KIND_FFM || wide_rows()) ? nb : 1; }
  // P, w and the scalars live back to back in ONE allocation ([P | w | scalars], each padded to 256 B,
  // padding zero) so the data-parallel exchange is a single collective over the arena
  DevBuf arena, lams;
  Span P, w, sc;
  bool initialized = false;
  // NFM_KIND_CFM (nfm_cfm_create): P [k][d] and lams [k] in the reference's layout, k = maxComponents; cfm_nc of them in use
  DevBuf cfm;
  int cfm_nc = 0;
  bool is_cfm() const { return cfg.kind == NFM_KIND_CFM; }
  CfmView cfm_view() const {
    CfmView v{};
    v.P = cfm.as<double>(); v.lams = cfm.as<double>() + (size_t)k * d; v.w = w.as<double>(); v.sc = sc.as<double>();
    v.d = d; v.max_components = k; v.n_components = cfm_nc; v.ignore_diag = cfg.reserved; v.fit_linear = cfg.fit_linear;
    v.fit_intercept = cfg.fit_intercept; v.task = cfg.task;
    return v;
  }
  ModelView view() const {
    ModelView m{};
    m.P = P.as<double>(); m.w = w.as<double>(); m.sc = sc.as<double>(); m.lams = lams.as<double>();
    m.d = d; m.da = da; m.nb = nb; m.k = kb; m.Kp = Kp; m.L = L; m.kc = kc;
    m.bs = bs_(); m.rs = rs_();
    m.degree = cfg.kind == NFM_KIND_FFM ? 2 : cfg.degree;
    m.n_aug = n_aug; m.kind = cfg.kind; m.fit_linear = cfg.fit_linear; m.fit_intercept = cfg.fit_intercept;
    m.task = cfg.task;
    return m;
  }
  int64_t nP() const { return (int64_t)nb * da * Kp; }
  int64_t n_ref() const { return (int64_t)no * k * da; }  // elements of the reference's P (and of each AdaGrad state tensor)
};

// ---- reference layouts <-> device blocks (util.hip does one block range at a time) ----
// FM parameters: reference [no][k][da] <-> device [no * kc][da][Kp]; block o * kc + c holds the factors c * kb ... of order o
static int fm_params_to_device(nfm_model* m, const double* src_ref, double* dst_dev) {
  if (m->kc == 1) return launch_fm_to_device(m->ctx, src_ref, dst_dev, m->nb, m->k, m->Kp, m->da);
  for (int o = 0; o < m->no; ++o)
    for (int c = 0; c < m->kc; ++c) {
      const int kk = std::min(m->kb, m->k - c * m->kb);
      NFM_TRY(launch_fm_to_device(m->ctx, src_ref + ((size_t)o * m->k + (size_t)c * m->kb) * m->da, dst_dev, 1, kk, m->Kp, m->da, m->bs_(),
                                  m->rs_(), o * m->kc + c));
    }
  return NFM_OK;
}
static int fm_params_from_device(nfm_model* m, const double* src_dev, double* dst_ref, const double* scale_dev) {
  if (m->kc == 1) return launch_fm_from_device(m->ctx, src_dev, dst_ref, m->nb, m->k, m->Kp, m->da, scale_dev);
  for (int o = 0; o < m->no; ++o)
    for (int c = 0; c < m->kc; ++c) {
      const int kk = std::min(m->kb, m->k - c * m->kb);
      NFM_TRY(launch_fm_from_device(m->ctx, src_dev, dst_ref + ((size_t)o * m->k + (size_t)c * m->kb) * m->da, 1, kk, m->Kp, m->da, scale_dev,
                                    m->bs_(), m->rs_(), o * m->kc + c));
    }
  return NFM_OK;
}
// row tensors in the training layout (AdaGrad state, gradients): reference [no * da][k] <-> device [nb * da][Kp]
static int rows_to_device(nfm_model* m, const double* src_ref, double* dst_dev, double pad) {
  const int major = m->cfg.kind == NFM_KIND_FFM ? m->nb : 0;  // (feature-major field rows, ModelView::row)
  if (m->kc == 1) return launch_rows_to_device(m->ctx, src_ref, dst_dev, (int64_t)m->nb * m->da, m->k, m->Kp, pad, major);
  return launch_rows_split_to_device(m->ctx, src_ref, dst_dev, m->no, m->da, m->k, m->kc, m->kb, m->Kp, pad, m->bs_(), m->rs_());
}
static int rows_from_device(nfm_model* m, const double* src_dev, double* dst_ref, const double* scale_dev) {
  const int major = m->cfg.kind == NFM_KIND_FFM ? m->nb : 0;
  if (m->kc == 1) return launch_rows_from_device(m->ctx, src_dev, dst_ref, (int64_t)m->nb * m->da, m->k, m->Kp, scale_dev, major);
  return launch_rows_split_from_device(m->ctx, src_dev, dst_ref, m->no, m->da, m->k, m->kc, m->kb, m->Kp, scale_dev, m->bs_(), m->rs_());
}

// ---- the batch plan of a mini-batch epoch call ----
// What a call needs its plan to have been built for: the one cache key, for the plan of the last call and for the plan
// built ahead alike.
struct PlanKey {
  uint64_t ds_uid;
  int64_t ds_nnz, begin, end, batch;
  bool first_singleton;
  int n_aug;
  bool use_singles;
};
static bool plan_is(const Plan& p, const PlanKey& k) {
  return p.ds_uid == k.ds_uid && p.ds_nnz == k.ds_nnz && p.begin == k.begin && p.end == k.end && p.batch == k.batch &&
         p.first_singleton == k.first_singleton && p.n_aug == k.n_aug && p.use_singles == k.use_singles;
}
// plan_build for a key, stamped with the dataset's identity (a plan without the stamp matches no later call: every call
// would build again).  perm_host, stream, perm_dev, csc and perm_key are plan_build's (plan.h).
static int build_plan(nfm_ctx* ctx, nfm_dataset* ds, const PlanKey& k, bool want_tq, bool sort_by_count, Plan* out, const int64_t* perm_host,
                      hipStream_t stream = nullptr, const int64_t* perm_dev = nullptr, CscIndex* csc = nullptr, const FeistelKey* perm_key = nullptr) {
  NFM_TRY(plan_build(ctx, ds->v, k.n_aug, perm_host, k.begin, k.end, k.batch, k.first_singleton, want_tq, k.use_singles, sort_by_count, out,
                     stream, perm_dev, csc, perm_key));
  out->ds_uid = ds->uid;
  out->ds_nnz = ds->v.nnz;
  return NFM_OK;
}

// The plan of the NEXT epoch call, built on a second stream while the current epoch runs: for the order the device will
// draw (nfm_opt_set_shuffle) or for the host's array announced for that call (nfm_opt_announce_perm).
struct PlanAhead {
  // the announcement: the host's permutation for the next call (kept alive by the caller) and the range it is for
  const int64_t* announced = nullptr;
  int64_t announced_begin = 0, announced_end = 0;
  // the plan built ahead; `ready`: it is complete, and nothing has happened since that it could be stale for
  std::unique_ptr<Plan> plan;
  bool ready = false;
  const int64_t* perm = nullptr;  // the host array it was built from; nullptr: from `order`, the device's draw of `epoch`
  int64_t probe[64] = {0};        // entries of that array at 64 evenly spaced places: it must come back unchanged
  DevBuf order;
  uint64_t epoch = 0;
  // made by the first call that builds ahead, released by nfm_opt_destroy
  hipStream_t stream = nullptr;
  double* out2_pinned = nullptr;  // where an epoch that is only enqueued (a build follows it) leaves its two sums

  static int64_t probe_at(const PlanKey& k, int q) { return k.begin + (k.end - k.begin - 1) * q / 63; }
  void offer(const int64_t* perm_next, int64_t begin, int64_t end) {
    announced = perm_next;
    announced_begin = begin;
    announced_end = end;
  }
  // the announcement, if it is for [begin, end); every mini-batch call uses it up
  const int64_t* take_offer(int64_t begin, int64_t end) {
    const int64_t* a = (announced && announced_begin == begin && announced_end == end) ? announced : nullptr;
    announced = nullptr;
    return a;
  }
  void invalidate() { ready = false; }
  // is the plan built ahead the plan of this call?  host_perm: the call's array (nullptr: the device's draw of shuffle_epoch)
  bool matches(const PlanKey& k, const int64_t* host_perm, uint64_t shuffle_epoch) const {
    if (!ready || !plan || perm != host_perm || !plan_is(*plan, k)) return false;
    if (!host_perm) return epoch == shuffle_epoch;
    for (int q = 0; q < 64; ++q)  // the array the plan was built from, unchanged as promised (a few probes)
      if (host_perm[probe_at(k, q)] != probe[q]) return false;
    return true;
  }
  void mark_ready(const PlanKey& k, const int64_t* from, uint64_t shuffle_epoch) {
    perm = from;
    if (from)
      for (int q = 0; q < 64; ++q) probe[q] = from[probe_at(k, q)];
    epoch = shuffle_epoch;
    ready = true;
  }
  int ensure_resources() {
    if (!out2_pinned) NFM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&out2_pinned), sizeof(double) * 2, hipHostMallocDefault));
    if (!stream) NFM_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return NFM_OK;
  }
  void release_resources() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    if (out2_pinned) (void)hipHostFree(out2_pinned);
  }
};

struct nfm_opt {
  nfm_ctx* ctx = nullptr;  // kept separately: the optimizer may outlive its model handle
  nfm_model* m = nullptr;  // valid only while model_of(o) finds m_uid among the live models
  uint64_t m_uid = 0;
  int kind = OPT_SGD, mode = NFM_MODE_SEQUENTIAL;
  int64_t batch = 1, it = 1;
  OptView o{};
  // AdaGrad state, one allocation [G | N | Gw | Nw | gscalars] (each padded to 256 B, padding zero)
  DevBuf state_arena, out2, perm_dev;
  Span G, N, Gw, Nw, gsc;
  bool state_ready = false;
  MbWork W;
  std::unique_ptr<Plan> plan;
  std::unique_ptr<SeqWin> seqwin;  // NFM_MODE_SEQUENTIAL: dependency table and mailboxes of the window kernel (seqwin.hip)
  // predictAllWithGrad: the one-batch plan of a dataset and its scratch, kept between calls (PGD-style solvers ask for
  // the full gradient of the same data once per iteration)
  MbWork Wg;
  std::unique_ptr<Plan> grad_plan;
  // device-side shuffle (nfm_opt_set_shuffle): every epoch call without an explicit permutation draws a fresh order on
  // the device
  int64_t shuffle_seed = -1;
  uint64_t shuffle_epoch = 0;
  DevBuf perm_gen;
  PlanAhead ahead;
  // data-parallel group (dp.h): when set, nfm_opt_epoch reconciles the replicas every dp_sync_period mini-batches
  // (delayed by one period when dp_overlap) and exactly at the end of the call
  nfm_dp* dp = nullptr;
  uint64_t dp_uid = 0;  // the group is checked against the live groups before every use (it may have been destroyed)
  int64_t dp_sync_period = 0;
  bool dp_overlap = true;
  int dp_combine = NFM_DP_AUTO;  // NFM_DP_AUTO: SGD the mean; AdaGrad summed at sync_period 1, its state increments averaged otherwise
  DevBuf dp_sums;
  // coordinate descent (nfm_cd_create): the level schedule of the dataset and the caches of the current fit (cd.h)
  std::unique_ptr<CdState> cd;
  CdParams cdp{};
  // PGD, FISTA, NMAPGD (nfm_pgd_create): the resident parameter sets and what the fit loops carry (pgd.h)
  std::unique_ptr<PgdState> pgd;
  // Katyusha (nfm_katyusha_create): the resident parameter sets of the current fit (katyusha.h)
  std::unique_ptr<KatState> kat;
  // Hazan (nfm_hazan_create): the column twin and the resident vectors of the current fit (cfm.h)
  std::unique_ptr<HazanState> hz;
  HazanCfg hzc{};
  // GreedyCD (nfm_gcd_create): the same for the convex model's other solver (gcd.h)
  std::unique_ptr<GcdState> gcd;
  GcdCfg gcdc{};
  // PSGD (nfm_psgd_create): the regulariser's lazy caches and psgd.nim's scalings_w, resident for the whole fit (psgd_seq.h)
  std::unique_ptr<PsgdSeqState> psgd;
};

// live models by uid: an optimizer whose model was destroyed (and whose address may since belong to a model of
// another shape) is refused instead of writing through a stale pointer
static std::mutex g_models_mu;
static std::map<uint64_t, nfm_model*> g_models;
static uint64_t register_model(nfm_model* m) {
  static uint64_t next = 0;
  std::lock_guard<std::mutex> lk(g_models_mu);
  g_models[++next] = m;
  return next;
}
static void unregister_model(uint64_t uid) {
  std::lock_guard<std::mutex> lk(g_models_mu);
  g_models.erase(uid);
}
static int model_of(nfm_opt* o, nfm_model** out) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  std::lock_guard<std::mutex> lk(g_models_mu);
  auto it = g_models.find(o->m_uid);
  NFM_CHECK(it != g_models.end() && it->second == o->m, NFM_ERR_INVALID,
            "the optimizer's model was destroyed; create the optimizer again for the new model");
  *out = it->second;
  return NFM_OK;
}

static int use_device(nfm_ctx* ctx) {
  NFM_HIP_CHECK(hipSetDevice(ctx->device));
  return NFM_OK;
}

extern "C" {

const char* nfm_last_error(void) { return nfm::last_error(); }
int32_t nfm_version(void) { return 100; }

int32_t nfm_device_count(int32_t* n) {
  NFM_CHECK(n, NFM_ERR_INVALID, "null out pointer");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return NFM_OK;
}

int32_t nfm_ctx_create(int32_t device_id, void* hip_stream, nfm_ctx** out) {
  NFM_CHECK(out, NFM_ERR_INVALID, "null out pointer");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess || c == 0)
    return set_error(NFM_ERR_HIP, "no HIP device available (%s); libnimfm_hip has no CPU fallback",
                     e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  NFM_CHECK(device_id >= 0 && device_id < c, NFM_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, c);
  std::unique_ptr<nfm_ctx> ctx(new nfm_ctx());
  ctx->device = device_id;
  NFM_HIP_CHECK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  NFM_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
  ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hip_stream) {
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  } else {
    NFM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  *out = ctx.release();
  return NFM_OK;
}

int32_t nfm_ctx_destroy(nfm_ctx* ctx) {
  if (!ctx) return NFM_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& p : ctx->timing.pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
  for (auto e : ctx->timing.pool) (void)hipEventDestroy(e);
  delete ctx->predict_pf;  // (the stream has drained)
  delete ctx->seq_scratch;
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return NFM_OK;
}

int32_t nfm_ctx_synchronize(nfm_ctx* ctx) {
  NFM_CHECK(ctx, NFM_ERR_INVALID, "null ctx");
  NFM_TRY(use_device(ctx));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return NFM_OK;
}

int32_t nfm_ctx_timing_enable(nfm_ctx* ctx, int32_t on) {
  NFM_CHECK(ctx, NFM_ERR_INVALID, "null ctx");
  NFM_TRY(timing_flush(ctx));
  ctx->timing.enabled = on != 0;
  return NFM_OK;
}
int32_t nfm_ctx_timing_reset(nfm_ctx* ctx) {
  NFM_CHECK(ctx, NFM_ERR_INVALID, "null ctx");
  NFM_TRY(timing_flush(ctx));
  ctx->timing.acc.clear();
  return NFM_OK;
}
int32_t nfm_ctx_timing_get(nfm_ctx* ctx, const char* family, int64_t* launches, double* total_ms) {
  NFM_CHECK(ctx && family, NFM_ERR_INVALID, "null argument");
  NFM_TRY(timing_flush(ctx));
  auto it = ctx->timing.acc.find(family);
  if (launches) *launches = it == ctx->timing.acc.end() ? 0 : it->second.launches;
  if (total_ms) *total_ms = it == ctx->timing.acc.end() ? 0.0 : it->second.ms;
  return NFM_OK;
}

// ------------------------------------------------------------------ dataset
static int validate_csr_host(int64_t n, int64_t d, const int64_t* indptr, const int64_t* indices, const int64_t* fields,
                             int64_t n_fields, int* max_row) {
  NFM_CHECK(n >= 0 && d >= 0, NFM_ERR_INVALID, "negative shape");
  NFM_CHECK(d < (int64_t)2147483647 - 64, NFM_ERR_UNSUPPORTED, "n_features must fit int32");
  NFM_CHECK(indptr, NFM_ERR_INVALID, "null indptr");
  NFM_CHECK(indptr[0] == 0, NFM_ERR_INVALID, "indptr[0] != 0");
  int64_t mr = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = indptr[i + 1] - indptr[i];
    NFM_CHECK(len >= 0, NFM_ERR_INVALID, "indptr not non-decreasing at row %lld", (long long)i);
    mr = std::max(mr, len);
  }
  NFM_CHECK(mr < (1 << 30), NFM_ERR_UNSUPPORTED, "row too long");
  const int64_t nnz = indptr[n];
  NFM_CHECK(nnz == 0 || indices, NFM_ERR_INVALID, "null indices");
  for (int64_t q = 0; q < nnz; ++q) {
    NFM_CHECK(indices[q] >= 0 && indices[q] < d, NFM_ERR_INVALID, "column index %lld out of range [0,%lld) at nnz %lld",
              (long long)indices[q], (long long)d, (long long)q);
    if (fields)
      NFM_CHECK(fields[q] >= 0 && fields[q] < n_fields, NFM_ERR_INVALID, "field %lld out of range [0,%lld) at nnz %lld",
                (long long)fields[q], (long long)n_fields, (long long)q);
  }
  *max_row = (int)mr;
  return NFM_OK;
}

int32_t nfm_dataset_create_csr(nfm_ctx* ctx, int64_t n, int64_t d, const int64_t* indptr, const int64_t* indices,
                               const double* data, const int64_t* fields, int64_t n_fields, const double* y,
                               nfm_dataset** out) {
  NFM_CHECK(ctx && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  int max_row = 0;
  NFM_TRY(validate_csr_host(n, d, indptr, indices, fields, n_fields, &max_row));
  const int64_t nnz = indptr[n];
  NFM_CHECK(nnz == 0 || data, NFM_ERR_INVALID, "null data");
  std::unique_ptr<nfm_dataset> ds(new nfm_dataset());
  ds->ctx = ctx;
  ds->uid = next_dataset_uid();
  ds->max_row = max_row;
  hipStream_t st = ctx->stream;
  NFM_TRY(ds->indptr.alloc(sizeof(int64_t) * (n + 1)));
  NFM_TRY(ds->indices.alloc(sizeof(int32_t) * nnz));
  NFM_TRY(ds->data.alloc(sizeof(double) * nnz));
  NFM_HIP_CHECK(hipMemcpyAsync(ds->indptr.p, indptr, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
  if (nnz > 0) {
    DevBuf wide;
    NFM_TRY(wide.alloc(sizeof(int64_t) * nnz));
    NFM_HIP_CHECK(hipMemcpyAsync(wide.p, indices, sizeof(int64_t) * nnz, hipMemcpyHostToDevice, st));
    NFM_TRY(launch_narrow_i64_i32(ctx, wide.as<int64_t>(), ds->indices.as<int32_t>(), nnz));
    if (fields) {
      NFM_TRY(ds->fields.alloc(sizeof(int32_t) * nnz));
      NFM_HIP_CHECK(hipMemcpyAsync(wide.p, fields, sizeof(int64_t) * nnz, hipMemcpyHostToDevice, st));
      NFM_TRY(launch_narrow_i64_i32(ctx, wide.as<int64_t>(), ds->fields.as<int32_t>(), nnz));
    }
    NFM_HIP_CHECK(hipMemcpyAsync(ds->data.p, data, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (y) {
    NFM_TRY(ds->y.alloc(sizeof(double) * n));
    NFM_HIP_CHECK(hipMemcpyAsync(ds->y.p, y, sizeof(double) * n, hipMemcpyHostToDevice, st));
    ds->has_y = true;
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  ds->v.indptr = ds->indptr.as<int64_t>();
  ds->v.indices = ds->indices.as<int32_t>();
  ds->v.data = ds->data.as<double>();
  ds->v.fields = fields ? ds->fields.as<int32_t>() : nullptr;
  ds->v.y = ds->has_y ? ds->y.as<double>() : nullptr;
  ds->v.n = n; ds->v.d = d; ds->v.nnz = nnz; ds->v.n_fields = fields ? (int32_t)n_fields : 0;
  ds->v.max_row = max_row;
  NFM_TRY(check_rows_distinct(ctx, ds->v, &ds->repeats, &ds->repeat_row, &ds->rows_ascend));
  *out = ds.release();
  return NFM_OK;
}

int32_t nfm_dataset_create_csr_device(nfm_ctx* ctx, int64_t n, int64_t d, int64_t nnz, const int64_t* indptr_dev,
                                      const int32_t* indices_dev, const double* data_dev, const int32_t* fields_dev,
                                      int64_t n_fields, const double* y_dev, nfm_dataset** out) {
  NFM_CHECK(ctx && out && indptr_dev, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(n >= 0 && d >= 0 && nnz >= 0 && d < (int64_t)2147483647 - 64, NFM_ERR_INVALID, "bad shape");
  NFM_CHECK(nnz == 0 || (indices_dev && data_dev), NFM_ERR_INVALID, "null indices/data");
  NFM_TRY(use_device(ctx));
  // the row-length bound needs indptr on the host once; values are trusted to be in range
  // (device-resident synthetic data); index range is checked by the caller's generator.
  std::vector<int64_t> ip((size_t)n + 1);
  NFM_HIP_CHECK(hipMemcpyAsync(ip.data(), indptr_dev, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  NFM_CHECK(ip[0] == 0 && ip[n] == nnz, NFM_ERR_INVALID, "indptr[0] != 0 or indptr[n] != nnz");
  int64_t mr = 0;
  for (int64_t i = 0; i < n; ++i) {
    NFM_CHECK(ip[i + 1] >= ip[i], NFM_ERR_INVALID, "indptr not non-decreasing at row %lld", (long long)i);
    mr = std::max(mr, ip[i + 1] - ip[i]);
  }
  std::unique_ptr<nfm_dataset> ds(new nfm_dataset());
  ds->ctx = ctx;
  ds->uid = next_dataset_uid();
  ds->max_row = (int)mr;
  ds->has_y = y_dev != nullptr;
  ds->v.indptr = indptr_dev; ds->v.indices = indices_dev; ds->v.data = data_dev; ds->v.fields = fields_dev;
  ds->v.y = y_dev; ds->v.n = n; ds->v.d = d; ds->v.nnz = nnz; ds->v.n_fields = fields_dev ? (int32_t)n_fields : 0;
  ds->v.max_row = (int32_t)mr;
  NFM_TRY(check_rows_distinct(ctx, ds->v, &ds->repeats, &ds->repeat_row, &ds->rows_ascend));
  *out = ds.release();
  return NFM_OK;
}

int32_t nfm_dataset_set_targets(nfm_dataset* ds, const double* y) {
  NFM_CHECK(ds && y, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ds->ctx));
  NFM_TRY(ds->y.ensure(sizeof(double) * ds->v.n));
  NFM_HIP_CHECK(hipMemcpyAsync(ds->y.p, y, sizeof(double) * ds->v.n, hipMemcpyHostToDevice, ds->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ds->ctx->stream));
  ds->has_y = true;
  ds->y_gen++;
  if (ds->v.y != ds->y.as<double>()) ds->serial++;  // a captured epoch graph holds the old pointer
  ds->v.y = ds->y.as<double>();
  return NFM_OK;
}

// ---- text ingest (ingest.hip) ----
static int dataset_from_ingest(nfm_ctx* ctx, IngestResult& r, bool with_fields, int64_t n_features, int64_t n_fields,
                               nfm_dataset** out) {
  // dataset.nim:623-631, 777-790: a given nFeatures / nFields smaller than what the file needs is an error,
  // a larger one wins
  if (n_features > 0 && r.d > n_features)
    return set_error(NFM_ERR_INVALID, "nFeatures is %lld but dataset has at least %lld features.", (long long)n_features,
                     (long long)r.d);
  if (with_fields && n_fields > 0 && r.n_fields > n_fields)
    return set_error(NFM_ERR_INVALID, "nFields is %lld but dataset has at least %lld fields.", (long long)n_fields,
                     (long long)r.n_fields);
  std::unique_ptr<nfm_dataset> ds(new nfm_dataset());
  ds->ctx = ctx;
  ds->uid = next_dataset_uid();
  ds->max_row = r.max_row;
  ds->indptr.take(r.indptr);
  ds->indices.take(r.indices);
  ds->data.take(r.data);
  ds->y.take(r.y);
  if (with_fields) ds->fields.take(r.fields);
  ds->has_y = true;
  ds->v.indptr = ds->indptr.as<int64_t>();
  ds->v.indices = ds->indices.as<int32_t>();
  ds->v.data = ds->data.as<double>();
  ds->v.fields = with_fields ? ds->fields.as<int32_t>() : nullptr;
  ds->v.y = ds->y.as<double>();
  ds->v.n = r.n;
  ds->v.d = std::max<int64_t>(r.d, n_features);
  ds->v.nnz = r.nnz;
  ds->v.n_fields = with_fields ? (int32_t)std::max<int64_t>(r.n_fields, n_fields) : 0;
  ds->v.max_row = r.max_row;
  ds->ingest_bytes = r.bytes;
  ds->ingest_upload_ms = r.upload_ms;
  ds->ingest_parse_ms = r.parse_ms;
  NFM_TRY(check_rows_distinct(ctx, ds->v, &ds->repeats, &ds->repeat_row, &ds->rows_ascend));
  *out = ds.release();
  return NFM_OK;
}

int32_t nfm_dataset_load_svmlight(nfm_ctx* ctx, const char* path, int64_t n_features, nfm_dataset** out) {
  NFM_CHECK(ctx && path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  IngestResult r;
  NFM_TRY(ingest_text(ctx, path, nullptr, 0, false, &r));
  return dataset_from_ingest(ctx, r, false, n_features, 0, out);
}

int32_t nfm_dataset_load_ffm(nfm_ctx* ctx, const char* path, int64_t n_features, int64_t n_fields, nfm_dataset** out) {
  NFM_CHECK(ctx && path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  IngestResult r;
  NFM_TRY(ingest_text(ctx, path, nullptr, 0, true, &r));
  return dataset_from_ingest(ctx, r, true, n_features, n_fields, out);
}

int32_t nfm_dataset_parse_text(nfm_ctx* ctx, const char* text, int64_t len, int32_t with_fields, int64_t n_features,
                               int64_t n_fields, nfm_dataset** out) {
  NFM_CHECK(ctx && out && len >= 0, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  IngestResult r;
  NFM_TRY(ingest_text(ctx, nullptr, text, len, with_fields != 0, &r));
  return dataset_from_ingest(ctx, r, with_fields != 0, n_features, n_fields, out);
}

int32_t nfm_dataset_load_stream(nfm_ctx* ctx, const char* x_path, const char* y_path, nfm_dataset** out) {
  NFM_CHECK(ctx && x_path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  IngestResult r;
  NFM_TRY(ingest_stream(ctx, x_path, y_path, &r));
  return dataset_from_ingest(ctx, r, r.n_fields > 0, -1, -1, out);
}

// ---- datasets made from datasets on the device (dataset_ops.hip) ----
static int dataset_from_parts(nfm_ctx* ctx, DsParts& r, nfm_dataset** out) {
  std::unique_ptr<nfm_dataset> ds(new nfm_dataset());
  ds->ctx = ctx;
  ds->uid = next_dataset_uid();
  ds->max_row = r.max_row;
  ds->indptr.take(r.indptr);
  ds->indices.take(r.indices);
  ds->data.take(r.data);
  if (r.has_fields) ds->fields.take(r.fields);
  if (r.has_y) ds->y.take(r.y);
  ds->has_y = r.has_y;
  ds->v.indptr = ds->indptr.as<int64_t>();
  ds->v.indices = ds->indices.as<int32_t>();
  ds->v.data = ds->data.as<double>();
  ds->v.fields = r.has_fields ? ds->fields.as<int32_t>() : nullptr;
  ds->v.y = r.has_y ? ds->y.as<double>() : nullptr;
  ds->v.n = r.n; ds->v.d = r.d; ds->v.nnz = r.nnz; ds->v.n_fields = r.has_fields ? (int32_t)r.n_fields : 0;
  ds->v.max_row = r.max_row;
  ds->ingest_bytes = r.bytes;
  ds->ingest_upload_ms = r.upload_ms;
  ds->ingest_parse_ms = r.parse_ms;
  NFM_TRY(check_rows_distinct(ctx, ds->v, &ds->repeats, &ds->repeat_row, &ds->rows_ascend));
  *out = ds.release();
  return NFM_OK;
}

// checkIndicesRow (dataset.nim:307-316) for the ids lo .. hi of m rows
static int check_indices_row(const nfm_dataset* ds, int64_t m, int64_t lo, int64_t hi) {
  NFM_CHECK(m >= 1, NFM_ERR_INVALID, "Invalid slice: nSamples < 1.");
  NFM_CHECK(hi < ds->v.n, NFM_ERR_INVALID, "max(indicesRow) %lld >= %lld.", (long long)hi, (long long)ds->v.n);
  NFM_CHECK(lo >= 0, NFM_ERR_INVALID, "min(indicesRow) %lld < 0.", (long long)lo);
  return NFM_OK;
}

int32_t nfm_dataset_select_rows(nfm_dataset* ds, const int64_t* rows, int64_t m, nfm_dataset** out) {
  NFM_CHECK(ds && out && (rows || m < 1), NFM_ERR_INVALID, "null argument");
  // tensor/sparse.nim:298
  NFM_TRY(refuse_csc(ds, "X[indices] (Accessing row vectors by openarray is not supported for CSCMatrix)"));
  int64_t lo = 0, hi = 0;
  if (m >= 1) {
    lo = *std::min_element(rows, rows + m);
    hi = *std::max_element(rows, rows + m);
  }
  NFM_TRY(check_indices_row(ds, m, lo, hi));
  NFM_TRY(use_device(ds->ctx));
  DsParts r;
  NFM_TRY(dsop_select_rows(ds->ctx, ds->v, rows, 0, m, &r));
  return dataset_from_parts(ds->ctx, r, out);
}

// ---- column-major datasets (dataset_csc.hip) ----
// n targets copied on the device
static int copy_targets(nfm_ctx* ctx, const double* src, int64_t n, DevBuf* dst) {
  NFM_TRY(dst->alloc(sizeof(double) * std::max<int64_t>(n, 1)));
  return dsop_copy(ctx, dst->p, src, sizeof(double) * n);
}

// the dataset of the column arrays `col` (as the transposed matrix: col.n = nFeatures, col.d = nSamples) and the targets y:
// makes the row twin and hands both to the new dataset
static int csc_from_columns(nfm_ctx* ctx, DsParts& col, DevBuf& y, bool has_y, nfm_dataset** out) {
  NFM_CHECK(col.d <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of %lld samples: sample ids are int32", (long long)col.d);
  CsrView cv{};
  cv.indptr = col.indptr.as<int64_t>(); cv.indices = col.indices.as<int32_t>(); cv.data = col.data.as<double>();
  cv.n = col.n; cv.d = col.d; cv.nnz = col.nnz; cv.max_row = col.max_row;
  DsParts row;
  NFM_TRY(dsop_transpose(ctx, cv, &row));
  if (has_y) row.y.take(y);
  row.has_y = has_y;
  nfm_dataset* ds = nullptr;
  NFM_TRY(dataset_from_parts(ctx, row, &ds));
  ds->layout = NFM_LAYOUT_CSC;
  ds->c_indptr.take(col.indptr);
  ds->c_indices.take(col.indices);
  ds->c_data.take(col.data);
  ds->cv = cv;
  *out = ds;
  return NFM_OK;
}

int32_t nfm_dataset_create_csc(nfm_ctx* ctx, int64_t n, int64_t d, const int64_t* indptr, const int64_t* indices, const double* data,
                               const double* y, nfm_dataset** out) {
  NFM_CHECK(ctx && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(n >= 0 && d >= 0, NFM_ERR_INVALID, "negative shape");
  NFM_CHECK(n <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of %lld samples: sample ids are int32", (long long)n);
  NFM_CHECK(d < (int64_t)2147483647 - 64, NFM_ERR_UNSUPPORTED, "n_features must fit int32");
  NFM_CHECK(indptr, NFM_ERR_INVALID, "null indptr");
  NFM_CHECK(indptr[0] == 0, NFM_ERR_INVALID, "indptr[0] != 0");
  int64_t mc = 0;
  for (int64_t j = 0; j < d; ++j) {
    NFM_CHECK(indptr[j + 1] >= indptr[j], NFM_ERR_INVALID, "indptr not non-decreasing at column %lld", (long long)j);
    mc = std::max(mc, indptr[j + 1] - indptr[j]);
  }
  const int64_t nnz = indptr[d];
  NFM_CHECK(nnz == 0 || (indices && data), NFM_ERR_INVALID, "null indices / data");
  for (int64_t q = 0; q < nnz; ++q)
    NFM_CHECK(indices[q] >= 0 && indices[q] < n, NFM_ERR_INVALID, "sample index %lld out of range [0,%lld) at nnz %lld", (long long)indices[q],
              (long long)n, (long long)q);
  NFM_CHECK(nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of more than 2^31-2 entries");
  NFM_TRY(use_device(ctx));
  hipStream_t st = ctx->stream;
  DsParts col;
  DevBuf wide, yb;
  NFM_TRY(col.indptr.alloc(sizeof(int64_t) * (d + 1)));
  NFM_TRY(dsop_alloc_entries(&col, nnz, false));
  NFM_HIP_CHECK(hipMemcpyAsync(col.indptr.p, indptr, sizeof(int64_t) * (d + 1), hipMemcpyHostToDevice, st));
  if (nnz > 0) {
    NFM_TRY(wide.alloc(sizeof(int64_t) * nnz));
    NFM_HIP_CHECK(hipMemcpyAsync(wide.p, indices, sizeof(int64_t) * nnz, hipMemcpyHostToDevice, st));
    NFM_TRY(launch_narrow_i64_i32(ctx, wide.as<int64_t>(), col.indices.as<int32_t>(), nnz));
    NFM_HIP_CHECK(hipMemcpyAsync(col.data.p, data, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
  }
  if (y) {
    NFM_TRY(yb.alloc(sizeof(double) * std::max<int64_t>(n, 1)));
    NFM_HIP_CHECK(hipMemcpyAsync(yb.p, y, sizeof(double) * n, hipMemcpyHostToDevice, st));
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  col.n = d; col.d = n; col.max_row = (int)std::min<int64_t>(mc, 2147483647);
  return csc_from_columns(ctx, col, yb, y != nullptr, out);
}

int32_t nfm_dataset_create_csc_device(nfm_ctx* ctx, int64_t n, int64_t d, int64_t nnz, const int64_t* indptr_dev, const int32_t* indices_dev,
                                      const double* data_dev, const double* y_dev, nfm_dataset** out) {
  NFM_CHECK(ctx && out && indptr_dev, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(n >= 0 && d >= 0 && nnz >= 0 && d < (int64_t)2147483647 - 64, NFM_ERR_INVALID, "bad shape");
  NFM_CHECK(n <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of %lld samples: sample ids are int32", (long long)n);
  NFM_CHECK(nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of more than 2^31-2 entries");
  NFM_CHECK(nnz == 0 || (indices_dev && data_dev), NFM_ERR_INVALID, "null indices/data");
  NFM_TRY(use_device(ctx));
  std::vector<int64_t> ip((size_t)d + 1);
  NFM_HIP_CHECK(hipMemcpyAsync(ip.data(), indptr_dev, sizeof(int64_t) * (d + 1), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  NFM_CHECK(ip[0] == 0 && ip[d] == nnz, NFM_ERR_INVALID, "indptr[0] != 0 or indptr[nFeatures] != nnz");
  int64_t mc = 0;
  for (int64_t j = 0; j < d; ++j) {
    NFM_CHECK(ip[j + 1] >= ip[j], NFM_ERR_INVALID, "indptr not non-decreasing at column %lld", (long long)j);
    mc = std::max(mc, ip[j + 1] - ip[j]);
  }
  DsParts col;
  DevBuf y;
  NFM_TRY(col.indptr.alloc(sizeof(int64_t) * (d + 1)));
  NFM_TRY(dsop_alloc_entries(&col, nnz, false));
  NFM_TRY(dsop_copy(ctx, col.indptr.p, indptr_dev, sizeof(int64_t) * (d + 1)));
  NFM_TRY(dsop_copy(ctx, col.indices.p, indices_dev, sizeof(int32_t) * nnz));
  NFM_TRY(dsop_copy(ctx, col.data.p, data_dev, sizeof(double) * nnz));
  if (y_dev) NFM_TRY(copy_targets(ctx, y_dev, n, &y));
  col.n = d; col.d = n; col.max_row = (int)std::min<int64_t>(mc, 2147483647);
  return csc_from_columns(ctx, col, y, y_dev != nullptr, out);
}

int32_t nfm_dataset_to_csc(nfm_dataset* ds, nfm_dataset** out) {
  NFM_CHECK(ds && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(ds->v.fields == nullptr, NFM_ERR_UNSUPPORTED, "toCSCDataset of a field-aware dataset: there is no CSCFieldDataset on the device");
  nfm_ctx* ctx = ds->ctx;
  NFM_TRY(use_device(ctx));
  DsParts col;
  DevBuf y;
  if (ds->layout == NFM_LAYOUT_CSC) {  // a copy
    NFM_TRY(col.indptr.alloc(sizeof(int64_t) * (ds->cv.n + 1)));
    NFM_TRY(dsop_alloc_entries(&col, ds->cv.nnz, false));
    NFM_TRY(dsop_copy(ctx, col.indptr.p, ds->cv.indptr, sizeof(int64_t) * (ds->cv.n + 1)));
    NFM_TRY(dsop_copy(ctx, col.indices.p, ds->cv.indices, sizeof(int32_t) * ds->cv.nnz));
    NFM_TRY(dsop_copy(ctx, col.data.p, ds->cv.data, sizeof(double) * ds->cv.nnz));
    col.n = ds->cv.n; col.d = ds->cv.d; col.max_row = ds->cv.max_row;
  } else {
    NFM_TRY(dsop_transpose(ctx, ds->v, &col));
  }
  if (ds->has_y) NFM_TRY(copy_targets(ctx, ds->v.y, ds->v.n, &y));
  return csc_from_columns(ctx, col, y, ds->has_y, out);
}

int32_t nfm_dataset_to_csr(nfm_dataset* ds, nfm_dataset** out) {
  NFM_CHECK(ds && out, NFM_ERR_INVALID, "null argument");
  nfm_ctx* ctx = ds->ctx;
  NFM_TRY(use_device(ctx));
  DsParts r;
  if (ds->layout == NFM_LAYOUT_CSC) {
    NFM_TRY(dsop_transpose(ctx, ds->cv, &r));
    if (ds->has_y) NFM_TRY(copy_targets(ctx, ds->v.y, ds->v.n, &r.y));
    r.has_y = ds->has_y;
  } else {
    NFM_TRY(dsop_select_rows(ctx, ds->v, nullptr, 0, ds->v.n, &r));  // a copy
  }
  return dataset_from_parts(ctx, r, out);
}

int32_t nfm_dataset_layout(const nfm_dataset* ds, int32_t* layout) {
  NFM_CHECK(ds && layout, NFM_ERR_INVALID, "null argument");
  *layout = ds->layout;
  return NFM_OK;
}

int32_t nfm_dataset_rows_ascend(const nfm_dataset* ds, int32_t* ascend) {
  NFM_CHECK(ds && ascend, NFM_ERR_INVALID, "null argument");
  *ascend = ds->rows_ascend ? 1 : 0;
  return NFM_OK;
}

int32_t nfm_dataset_get_csc(nfm_dataset* ds, int64_t* indptr, int64_t* indices, double* data) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  NFM_CHECK(ds->layout == NFM_LAYOUT_CSC, NFM_ERR_INVALID, "the dataset is row-major: nfm_dataset_get_csr reads it (or convert it with nfm_dataset_to_csc)");
  NFM_TRY(use_device(ds->ctx));
  hipStream_t st = ds->ctx->stream;
  const int64_t d = ds->cv.n, nnz = ds->cv.nnz;
  if (indptr) NFM_HIP_CHECK(hipMemcpyAsync(indptr, ds->cv.indptr, sizeof(int64_t) * (d + 1), hipMemcpyDeviceToHost, st));
  if (data && nnz) NFM_HIP_CHECK(hipMemcpyAsync(data, ds->cv.data, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
  if (indices && nnz) {
    std::vector<int32_t> tmp((size_t)nnz);
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.data(), ds->cv.indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t q = 0; q < nnz; ++q) indices[q] = tmp[q];
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

int32_t nfm_dataset_slice_rows(nfm_dataset* ds, int64_t begin, int64_t end, nfm_dataset** out) {
  NFM_CHECK(ds && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(check_indices_row(ds, end - begin, begin, end - 1));
  NFM_TRY(use_device(ds->ctx));
  if (ds->layout == NFM_LAYOUT_CSC) {  // tensor/sparse.nim:300-325
    DsParts col;
    DevBuf y;
    NFM_TRY(dsop_filter_minor(ds->ctx, ds->cv, begin, end, &col));
    if (ds->has_y) NFM_TRY(copy_targets(ds->ctx, ds->v.y + begin, end - begin, &y));
    return csc_from_columns(ds->ctx, col, y, ds->has_y, out);
  }
  DsParts r;
  NFM_TRY(dsop_select_rows(ds->ctx, ds->v, nullptr, begin, end - begin, &r));
  return dataset_from_parts(ds->ctx, r, out);
}

static int stack_views(nfm_dataset* const* parts, int64_t n_parts, nfm_dataset** out, std::vector<CsrView>* views) {
  NFM_CHECK(parts && out && n_parts >= 1 && n_parts < (1 << 20), NFM_ERR_INVALID, "null argument or no parts");
  for (int64_t p = 0; p < n_parts; ++p) {
    NFM_CHECK(parts[p], NFM_ERR_INVALID, "null dataset");
    NFM_CHECK(parts[p]->ctx == parts[0]->ctx, NFM_ERR_INVALID, "the datasets belong to different contexts");
    NFM_CHECK((parts[p]->v.fields != nullptr) == (parts[0]->v.fields != nullptr), NFM_ERR_INVALID,
              "plain and field-aware datasets cannot be stacked together");
    NFM_CHECK(parts[p]->layout == parts[0]->layout, NFM_ERR_INVALID,
              "row-major and column-major datasets cannot be stacked together (convert with toCSRDataset / toCSCDataset)");
    views->push_back(parts[p]->layout == NFM_LAYOUT_CSC ? parts[p]->cv : parts[p]->v);
  }
  return NFM_OK;
}

// The stacks of column-major parts are the other stack of the transposed views (dataset_ops.h): `stack` is dsop_hstack for
// vstack and dsop_vstack for hstack.  The targets: concatenated when every part has them (vstack), the first part's (hstack).
static int csc_stack(nfm_dataset* const* parts, std::vector<CsrView>& v, bool vertical, nfm_dataset** out) {
  nfm_ctx* ctx = parts[0]->ctx;
  int64_t n = 0, d = 0;
  bool all_y = true;
  for (size_t p = 0; p < v.size(); ++p) {
    if (vertical)
      NFM_CHECK(v[p].n == v[0].n, NFM_ERR_INVALID, "All matrics must have the same shape[1].");  // tensor/sparse.nim:592
    else
      NFM_CHECK(v[p].d == v[0].d, NFM_ERR_INVALID, "All matrics must have the same shape[0]");  // :712, as written there
    n += v[p].d;
    d += v[p].n;
    all_y = all_y && parts[p]->has_y;
  }
  if (vertical)
    NFM_CHECK(n <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of %lld samples: sample ids are int32", (long long)n);
  else
    NFM_CHECK(d < (int64_t)2147483647 - 64, NFM_ERR_UNSUPPORTED, "n_features must fit int32");
  NFM_TRY(use_device(ctx));
  DsParts col;
  DevBuf y;
  bool has_y = false;
  if (vertical) {
    NFM_TRY(dsop_hstack(ctx, v.data(), (int)v.size(), &col));
    if (all_y) {
      NFM_TRY(y.alloc(sizeof(double) * std::max<int64_t>(n, 1)));
      int64_t r0 = 0;
      for (size_t p = 0; p < v.size(); ++p) {
        NFM_TRY(dsop_copy(ctx, y.as<double>() + r0, parts[p]->v.y, sizeof(double) * parts[p]->v.n));
        r0 += parts[p]->v.n;
      }
      has_y = true;
    }
  } else {
    NFM_TRY(dsop_vstack(ctx, v.data(), (int)v.size(), &col));
    if (parts[0]->has_y) {
      NFM_TRY(copy_targets(ctx, parts[0]->v.y, parts[0]->v.n, &y));
      has_y = true;
    }
  }
  return csc_from_columns(ctx, col, y, has_y, out);
}

int32_t nfm_dataset_vstack(nfm_dataset* const* parts, int64_t n_parts, nfm_dataset** out) {
  std::vector<CsrView> v;
  NFM_TRY(stack_views(parts, n_parts, out, &v));
  if (parts[0]->layout == NFM_LAYOUT_CSC) return csc_stack(parts, v, true, out);
  for (const CsrView& x : v) NFM_CHECK(x.d == v[0].d, NFM_ERR_INVALID, "All matrics must have the same shape[1].");
  NFM_TRY(use_device(parts[0]->ctx));
  DsParts r;
  NFM_TRY(dsop_vstack(parts[0]->ctx, v.data(), (int)v.size(), &r));
  return dataset_from_parts(parts[0]->ctx, r, out);
}

int32_t nfm_dataset_hstack(nfm_dataset* const* parts, int64_t n_parts, nfm_dataset** out) {
  std::vector<CsrView> v;
  NFM_TRY(stack_views(parts, n_parts, out, &v));
  if (parts[0]->layout == NFM_LAYOUT_CSC) return csc_stack(parts, v, false, out);
  int64_t d = 0, nf = 0;
  for (const CsrView& x : v) {
    NFM_CHECK(x.n == v[0].n, NFM_ERR_INVALID, "All matrics must have the same shape[0].");
    d += x.d;
    nf += x.n_fields;
    NFM_CHECK(d < (int64_t)2147483647 - 64 && nf < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "n_features must fit int32");
  }
  NFM_TRY(use_device(parts[0]->ctx));
  DsParts r;
  NFM_TRY(dsop_hstack(parts[0]->ctx, v.data(), (int)v.size(), &r));
  return dataset_from_parts(parts[0]->ctx, r, out);
}

int32_t nfm_dataset_normalize(nfm_dataset* ds, int32_t axis, int32_t norm, nfm_dataset** out) {
  NFM_CHECK(ds && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(axis == 0 || axis == 1, NFM_ERR_INVALID, "axis must be 0 or 1");
  NFM_CHECK(norm == NFM_NORM_L1 || norm == NFM_NORM_L2 || norm == NFM_NORM_LINFTY, NFM_ERR_INVALID, "bad norm kind");
  NFM_TRY(use_device(ds->ctx));
  if (ds->layout == NFM_LAYOUT_CSC) {  // tensor/sparse.nim:414-427: the same fold with 1 - axis on the column arrays
    DsParts col;
    DevBuf y;
    NFM_TRY(dsop_normalize(ds->ctx, ds->cv, 1 - axis, norm, &col));
    if (ds->has_y) NFM_TRY(copy_targets(ds->ctx, ds->v.y, ds->v.n, &y));
    return csc_from_columns(ds->ctx, col, y, ds->has_y, out);
  }
  DsParts r;
  NFM_TRY(dsop_normalize(ds->ctx, ds->v, axis, norm, &r));
  return dataset_from_parts(ds->ctx, r, out);
}

int32_t nfm_dataset_load_user_item(nfm_ctx* ctx, const char* path, nfm_dataset** out) {
  NFM_CHECK(ctx && path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  DsParts r;
  NFM_TRY(dsop_user_item(ctx, path, nullptr, 0, &r));
  return dataset_from_parts(ctx, r, out);
}

int32_t nfm_dataset_parse_user_item(nfm_ctx* ctx, const char* text, int64_t len, nfm_dataset** out) {
  NFM_CHECK(ctx && out && len >= 0, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  DsParts r;
  NFM_TRY(dsop_user_item(ctx, nullptr, text, len, &r));
  return dataset_from_parts(ctx, r, out);
}

int32_t nfm_dataset_load_user_item_lines(nfm_ctx* ctx, const char* path, int32_t short_lines, nfm_dataset** out) {
  NFM_CHECK(ctx && path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  DsParts r;
  NFM_TRY(dsop_user_item(ctx, path, nullptr, 0, &r, short_lines != 0));
  return dataset_from_parts(ctx, r, out);
}

int32_t nfm_dataset_parse_user_item_lines(nfm_ctx* ctx, const char* text, int64_t len, int32_t short_lines, nfm_dataset** out) {
  NFM_CHECK(ctx && out && len >= 0, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  DsParts r;
  NFM_TRY(dsop_user_item(ctx, nullptr, text, len, &r, short_lines != 0));
  return dataset_from_parts(ctx, r, out);
}

// ---- a dataset on the device -> its text file (dataset_text.hip) ----
static thread_local TextStats g_dump_stats;  // of this thread's last nfm_dataset_dump_* / nfm_dataset_format_text

static int dump_checks(nfm_dataset* ds, const double* y, int want_fields) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  NFM_TRY(refuse_csc(ds, want_fields < 0 ? "formatText" : want_fields ? "dumpFFMFile" : "dumpSVMLightFile"));
  NFM_CHECK(want_fields < 0 || (ds->v.fields != nullptr) == (want_fields != 0), NFM_ERR_INVALID,
            want_fields ? "dumpFFMFile needs a field-aware dataset" : "dumpSVMLightFile needs a dataset without fields (dumpFFMFile writes those)");
  NFM_CHECK(y || ds->has_y, NFM_ERR_INVALID, "X.nSamples != len(y).");  // dataset.nim:796, 828
  return NFM_OK;
}

static int dump_to_path(nfm_dataset* ds, const char* path, const double* y, int32_t y_int, int64_t chunk_bytes, int want_fields) {
  NFM_CHECK(path, NFM_ERR_INVALID, "null argument");
  NFM_TRY(dump_checks(ds, y, want_fields));
  NFM_TRY(use_device(ds->ctx));
  TextSink sink;
  sink.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  NFM_CHECK(sink.fd >= 0, NFM_ERR_INVALID, "%s cannot be written.", path);
  int64_t len = 0;
  const int rc = format_dataset_text(ds->ctx, ds->v, y, y_int != 0, chunk_bytes, sink, &len, &g_dump_stats);
  const bool closed = close(sink.fd) == 0;
  if (rc != NFM_OK) return rc;
  NFM_CHECK(closed, NFM_ERR_INVALID, "%s cannot be written.", path);
  return NFM_OK;
}

int32_t nfm_dataset_dump_svmlight(nfm_dataset* ds, const char* path, const double* y, int32_t y_int, int64_t chunk_bytes) {
  return dump_to_path(ds, path, y, y_int, chunk_bytes, 0);
}

int32_t nfm_dataset_dump_ffm(nfm_dataset* ds, const char* path, const double* y, int32_t y_int, int64_t chunk_bytes) {
  return dump_to_path(ds, path, y, y_int, chunk_bytes, 1);
}

int32_t nfm_dataset_format_text(nfm_dataset* ds, const double* y, int32_t y_int, int64_t chunk_bytes, char* buf, int64_t cap, int64_t* len) {
  NFM_CHECK(len && (!buf || cap >= 0), NFM_ERR_INVALID, "null argument");
  NFM_TRY(dump_checks(ds, y, -1));
  NFM_TRY(use_device(ds->ctx));
  TextSink sink;
  char none = 0;
  if (buf) {
    sink.buf = cap > 0 ? buf : &none;
    sink.cap = cap;
  }
  return format_dataset_text(ds->ctx, ds->v, y, y_int != 0, chunk_bytes, sink, len, &g_dump_stats);
}

int32_t nfm_dump_stats(int64_t* pieces, int64_t* bytes, double* copy_ms, double* sink_ms, double* total_ms) {
  if (pieces) *pieces = g_dump_stats.pieces;
  if (bytes) *bytes = g_dump_stats.bytes;
  if (copy_ms) *copy_ms = g_dump_stats.copy_ms;
  if (sink_ms) *sink_ms = g_dump_stats.sink_ms;
  if (total_ms) *total_ms = g_dump_stats.total_ms;
  return NFM_OK;
}

// ---- a dataset on the device -> its binary stream file, and the files made from files (dataset_stream.hip, DESIGN.md
// section 30) ----
// row-major plain -> STREAMCSR, field-aware -> STREAMCSRFIELD, column-major -> STREAMCSC (its column arrays); the header's
// nRows / nCols are n_samples / n_features in every case
static int stream_dump(nfm_dataset* ds, int64_t chunk_bytes, const TextSink& sink, int64_t* len) {
  const bool csc = ds->layout == NFM_LAYOUT_CSC;
  const CsrView& X = csc ? ds->cv : ds->v;
  const int kind = csc ? STREAM_CSC : X.fields ? STREAM_CSRFIELD : STREAM_CSR;
  double vmax = 0.0, vmin = 0.0;
  NFM_TRY(stream_minmax(ds->ctx, X.data, X.nnz, &vmax, &vmin));
  char head[kStreamHeadMax];
  const int head_len = stream_head(kind, ds->v.n, ds->v.d, ds->v.nnz, ds->v.n_fields, vmax, vmin, head);
  return pack_stream(ds->ctx, X, 0, 0, head, head_len, chunk_bytes, sink, len, &g_dump_stats);
}

int32_t nfm_dataset_dump_stream(nfm_dataset* ds, const char* path, int64_t chunk_bytes) {
  NFM_CHECK(ds && path, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ds->ctx));
  TextSink sink;
  sink.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  NFM_CHECK(sink.fd >= 0, NFM_ERR_INVALID, "%s cannot be written.", path);
  int64_t len = 0;
  const int rc = stream_dump(ds, chunk_bytes, sink, &len);
  const bool closed = close(sink.fd) == 0;
  if (rc != NFM_OK) return rc;
  NFM_CHECK(closed, NFM_ERR_INVALID, "%s cannot be written.", path);
  return NFM_OK;
}

int32_t nfm_dataset_format_stream(nfm_dataset* ds, int64_t chunk_bytes, char* buf, int64_t cap, int64_t* len) {
  NFM_CHECK(ds && len && (!buf || cap >= 0), NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ds->ctx));
  TextSink sink;
  char none = 0;
  if (buf) {
    sink.buf = cap > 0 ? buf : &none;
    sink.cap = cap;
  }
  return stream_dump(ds, chunk_bytes, sink, len);
}

int32_t nfm_dataset_load_stream_csc(nfm_ctx* ctx, const char* x_path, const char* y_path, nfm_dataset** out) {
  NFM_CHECK(ctx && x_path && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  IngestResult r;
  NFM_TRY(ingest_stream_csc(ctx, x_path, y_path, &r));
  NFM_CHECK(r.nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "a CSCDataset of more than 2^31-2 entries");
  DsParts col;
  col.indptr.take(r.indptr);
  col.indices.take(r.indices);
  col.data.take(r.data);
  col.n = r.n; col.d = r.d; col.nnz = r.nnz; col.max_row = r.max_row;
  return csc_from_columns(ctx, col, r.y, true, out);
}

int32_t nfm_transpose_file(nfm_ctx* ctx, const char* f_in, const char* f_out, int64_t chunk_bytes) {
  NFM_CHECK(ctx && f_in && f_out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  char magic[14] = {0};
  {
    FILE* f = fopen(f_in, "rb");
    NFM_CHECK(f, NFM_ERR_INVALID, "%s cannot be read.", f_in);
    const size_t got = fread(magic, 1, sizeof(magic), f);
    fclose(f);
    if (got < sizeof(magic)) memset(magic + got, 0, sizeof(magic) - got);
  }
  const bool csr = !memcmp(magic, "STREAMCSR", 9), csc = !memcmp(magic, "STREAMCSC", 9);
  NFM_CHECK(csr || csc, NFM_ERR_INVALID, "%s is not neither StreamCSC nor StreamCSR file.", f_in);
  // the reference compares 9 bytes only and would read a field-aware file's 48-byte header and 24-byte elements as plain ones
  NFM_CHECK(memcmp(magic + 9, "FIELD", 5) != 0, NFM_ERR_UNSUPPORTED,
            "%s is a field-aware (...FIELD) file: transposeFile reads plain StreamCSR / StreamCSC files only", f_in);
  IngestResult r;
  unsigned char hdr40[40];
  NFM_TRY(csr ? ingest_stream(ctx, f_in, nullptr, &r, hdr40) : ingest_stream_csc(ctx, f_in, nullptr, &r, hdr40));
  // what nfm_dataset_to_csc can take: int32 ids and entry counts
  NFM_CHECK(r.nnz < (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "transposeFile of more than 2^31-2 entries");
  NFM_CHECK(r.n <= (int64_t)2147483647, NFM_ERR_UNSUPPORTED, "transposeFile of %lld records: their ids are int32", (long long)r.n);
  CsrView in{};
  in.indptr = r.indptr.as<int64_t>(); in.indices = r.indices.as<int32_t>(); in.data = r.data.as<double>();
  in.n = r.n; in.d = r.d; in.nnz = r.nnz; in.max_row = r.max_row;
  // dataset.nim:1150, 1190-1196: the count of output record 0 is written, then decremented per element and `j` advances only
  // when it reaches 0 -- from 0 it goes negative and the loop over `j` never ends
  const char* kEmptyFirst = "%s: the first record of the transposed file would be empty; the reference's transposeFile does not terminate on such a file";
  NFM_CHECK(r.d > 0 && r.nnz > 0, NFM_ERR_INVALID, kEmptyFirst, f_in);
  DsParts t;
  NFM_TRY(dsop_transpose(ctx, in, &t));
  int64_t first[2] = {0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(first, t.indptr.p, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  NFM_CHECK(first[1] - first[0] > 0, NFM_ERR_INVALID, kEmptyFirst, f_in);
  CsrView tv{};
  tv.indptr = t.indptr.as<int64_t>(); tv.indices = t.indices.as<int32_t>(); tv.data = t.data.as<double>();
  tv.n = r.d; tv.d = r.n; tv.nnz = r.nnz;
  // the other magic, then the input's header as it is (:1122-1124): max / min are not recomputed, nRows / nCols not swapped
  char head[kStreamHeadMax];
  memcpy(head, csr ? "STREAMCSC" : "STREAMCSR", 9);
  memcpy(head + 9, hdr40, 40);
  TextSink sink;
  sink.fd = open(f_out, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  NFM_CHECK(sink.fd >= 0, NFM_ERR_INVALID, "%s cannot be read.", f_out);  // the reference's wording for fOut (dataset.nim:1108-1109)
  int64_t len = 0;
  const int rc = pack_stream(ctx, tv, 0, 0, head, 49, chunk_bytes, sink, &len, &g_dump_stats);
  const bool closed = close(sink.fd) == 0;
  if (rc != NFM_OK) return rc;
  NFM_CHECK(closed, NFM_ERR_INVALID, "%s cannot be written.", f_out);
  return NFM_OK;
}

int32_t nfm_convert_ffm(nfm_ctx* ctx, const char* f_in, const char* f_out_x, const char* f_out_y) {
  NFM_CHECK(ctx && f_in && f_out_x && f_out_y, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  return convert_ffm(ctx, f_in, f_out_x, f_out_y);
}

int32_t nfm_format_f64(nfm_ctx* ctx, const double* values, int64_t n_rows, int64_t row_len, char* buf, int64_t cap, int64_t* len) {
  NFM_CHECK(ctx && len && n_rows >= 0 && row_len >= 0 && (values || n_rows * row_len == 0) && (!buf || cap >= 0), NFM_ERR_INVALID,
            "null argument or negative shape");
  NFM_TRY(use_device(ctx));
  return format_f64_text(ctx, values, n_rows, row_len, buf, cap, len);
}

static thread_local TextStats g_parse_stats;  // of this thread's last nfm_parse_f64

int32_t nfm_parse_f64(nfm_ctx* ctx, const char* text, int64_t len, int64_t n_rows, int64_t row_len, int64_t chunk_bytes, double* values,
                      int64_t* consumed, int32_t* clean) {
  NFM_CHECK(ctx && consumed && clean && len >= 0 && (text || len == 0) && n_rows >= 0 && row_len >= 0 && chunk_bytes >= 0, NFM_ERR_INVALID,
            "null argument or negative shape");
  NFM_CHECK(row_len == 0 || n_rows <= (INT64_MAX / 8) / row_len, NFM_ERR_INVALID, "n_rows * row_len does not fit");
  NFM_CHECK(values || n_rows * row_len == 0, NFM_ERR_INVALID, "null argument or negative shape");
  NFM_TRY(use_device(ctx));
  return parse_f64_text(ctx, text, len, n_rows, row_len, chunk_bytes, values, consumed, clean, &g_parse_stats);
}

int32_t nfm_parse_stats(int64_t* pieces, int64_t* bytes, double* copy_ms, double* sink_ms, double* total_ms) {
  if (pieces) *pieces = g_parse_stats.pieces;
  if (bytes) *bytes = g_parse_stats.bytes;
  if (copy_ms) *copy_ms = g_parse_stats.copy_ms;
  if (sink_ms) *sink_ms = g_parse_stats.sink_ms;
  if (total_ms) *total_ms = g_parse_stats.total_ms;
  return NFM_OK;
}

struct nfm_stream {
  nfm_ctx* ctx = nullptr;
  StreamFile f;
  // One row block loaded ahead (nfm_stream_prefetch_rows) by a thread of the stream object's own -- ONE thread for all
  // blocks: the device-memory cache hands a thread its own released blocks back without a device-wide wait (util.hip),
  // so the block-sized staging buffer of the previous load is reused while the caller's epoch is still running -- on a
  // HIP stream of its own.
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv;
  bool job = false, busy = false, quit = false;
  hipStream_t pf_stream = nullptr;
  bool pf_active = false;
  int64_t pf_r0 = 0, pf_r1 = 0;
  int pf_rc = NFM_OK;
  std::string pf_err;
  std::unique_ptr<IngestResult> pf_res;
  void run() {
    if (hipSetDevice(ctx->device) != hipSuccess) {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
      busy = false;
      pf_rc = NFM_ERR_HIP;
      pf_err = "the prefetch thread could not select the context's device";
      cv.notify_all();
      return;
    }
    std::unique_lock<std::mutex> lk(mu);
    while (true) {
      cv.wait(lk, [&] { return job || quit; });
      if (quit) return;
      job = false;
      lk.unlock();
      const int rc = f.load_rows(ctx, pf_r0, pf_r1, pf_res.get(), pf_stream);
      std::string err = rc != NFM_OK ? nfm_last_error() : "";  // (the message lives in this thread's slot)
      lk.lock();
      pf_rc = rc;
      pf_err = err;
      busy = false;
      cv.notify_all();
    }
  }
  void join() {  // until the block being loaded, if any, is there
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy; });
  }
  ~nfm_stream() {
    join();
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    if (worker.joinable()) worker.join();
    pf_res.reset();
    if (pf_stream) (void)hipStreamDestroy(pf_stream);
  }
};

int32_t nfm_stream_open(nfm_ctx* ctx, const char* x_path, const char* y_path, nfm_stream** out) {
  NFM_CHECK(ctx && x_path && out, NFM_ERR_INVALID, "null argument");
  std::unique_ptr<nfm_stream> s(new nfm_stream());
  s->ctx = ctx;
  NFM_TRY(StreamFile::open_file(x_path, y_path, &s->f));
  *out = s.release();
  return NFM_OK;
}

int32_t nfm_stream_shape(const nfm_stream* s, int64_t* n_samples, int64_t* n_features, int64_t* nnz, int64_t* n_fields) {
  NFM_CHECK(s, NFM_ERR_INVALID, "null stream");
  if (n_samples) *n_samples = s->f.n;
  if (n_features) *n_features = s->f.d;
  if (nnz) *nnz = s->f.nnz;
  if (n_fields) *n_fields = s->f.nf;
  return NFM_OK;
}

int32_t nfm_stream_prefetch_rows(nfm_stream* s, int64_t row_begin, int64_t row_end) {
  NFM_CHECK(s, NFM_ERR_INVALID, "null stream");
  NFM_CHECK(row_begin >= 0 && row_begin <= row_end && row_end <= s->f.n, NFM_ERR_INVALID, "rows [%lld,%lld) outside [0,%lld)",
            (long long)row_begin, (long long)row_end, (long long)s->f.n);
  NFM_TRY(use_device(s->ctx));
  s->join();  // at most one block ahead; an unclaimed one is dropped
  s->pf_res.reset();
  if (!s->pf_stream) NFM_HIP_CHECK(hipStreamCreateWithFlags(&s->pf_stream, hipStreamNonBlocking));
  s->pf_active = true;
  s->pf_r0 = row_begin;
  s->pf_r1 = row_end;
  s->pf_rc = NFM_OK;
  s->pf_err.clear();
  s->pf_res.reset(new IngestResult());
  if (!s->worker.joinable()) s->worker = std::thread([s]() { s->run(); });
  {
    std::lock_guard<std::mutex> lk(s->mu);
    NFM_CHECK(!s->quit, NFM_ERR_HIP, "the prefetch thread could not select device %d", s->ctx->device);
    s->job = true;
    s->busy = true;
  }
  s->cv.notify_all();
  return NFM_OK;
}

int32_t nfm_stream_load_rows(nfm_stream* s, int64_t row_begin, int64_t row_end, nfm_dataset** out) {
  NFM_CHECK(s && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(s->ctx));
  s->join();
  if (s->pf_active && s->pf_r0 == row_begin && s->pf_r1 == row_end) {  // the block asked for ahead
    s->pf_active = false;
    std::unique_ptr<IngestResult> r(std::move(s->pf_res));
    if (s->pf_rc != NFM_OK) return set_error(s->pf_rc, "%s", s->pf_err.c_str());
    return dataset_from_ingest(s->ctx, *r, r->n_fields > 0, -1, -1, out);
  }
  s->pf_active = false;
  s->pf_res.reset();
  IngestResult r;
  NFM_TRY(s->f.load_rows(s->ctx, row_begin, row_end, &r));
  return dataset_from_ingest(s->ctx, r, r.n_fields > 0, -1, -1, out);
}

int32_t nfm_stream_close(nfm_stream* s) {
  if (s && use_device(s->ctx) != NFM_OK) return NFM_ERR_HIP;
  delete s;
  return NFM_OK;
}

int32_t nfm_convert_svmlight(nfm_ctx* ctx, const char* f_in, const char* f_out_x, const char* f_out_y) {
  NFM_CHECK(ctx && f_in && f_out_x && f_out_y, NFM_ERR_INVALID, "null argument");
  NFM_TRY(use_device(ctx));
  return convert_svmlight(ctx, f_in, f_out_x, f_out_y);
}

int32_t nfm_dataset_shape(const nfm_dataset* ds, int64_t* n_samples, int64_t* n_features, int64_t* nnz, int64_t* n_fields) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  if (n_samples) *n_samples = ds->v.n;
  if (n_features) *n_features = ds->v.d;
  if (nnz) *nnz = ds->v.nnz;
  if (n_fields) *n_fields = ds->v.n_fields;
  return NFM_OK;
}

int32_t nfm_dataset_ingest_stats(const nfm_dataset* ds, int64_t* bytes, double* upload_ms, double* parse_ms) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  if (bytes) *bytes = ds->ingest_bytes;
  if (upload_ms) *upload_ms = ds->ingest_upload_ms;
  if (parse_ms) *parse_ms = ds->ingest_parse_ms;
  return NFM_OK;
}

int32_t nfm_dataset_get_targets(nfm_dataset* ds, double* y) {
  NFM_CHECK(ds && y, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "the dataset has no targets");
  NFM_TRY(use_device(ds->ctx));
  NFM_HIP_CHECK(hipMemcpyAsync(y, ds->v.y, sizeof(double) * ds->v.n, hipMemcpyDeviceToHost, ds->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ds->ctx->stream));
  return NFM_OK;
}

int32_t nfm_dataset_get_csr(nfm_dataset* ds, int64_t* indptr, int64_t* indices, double* data, int64_t* fields) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  NFM_TRY(use_device(ds->ctx));
  hipStream_t st = ds->ctx->stream;
  const int64_t n = ds->v.n, nnz = ds->v.nnz;
  if (indptr) NFM_HIP_CHECK(hipMemcpyAsync(indptr, ds->v.indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, st));
  if (data && nnz) NFM_HIP_CHECK(hipMemcpyAsync(data, ds->v.data, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
  std::vector<int32_t> tmp;
  if ((indices || fields) && nnz) tmp.resize((size_t)nnz);
  if (indices && nnz) {
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.data(), ds->v.indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t q = 0; q < nnz; ++q) indices[q] = tmp[q];
  }
  if (fields && nnz) {
    NFM_CHECK(ds->v.fields, NFM_ERR_INVALID, "the dataset has no fields");
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.data(), ds->v.fields, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t q = 0; q < nnz; ++q) fields[q] = tmp[q];
  }
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

int32_t nfm_dataset_destroy(nfm_dataset* ds) {
  if (!ds) return NFM_OK;
  (void)hipSetDevice(ds->ctx->device);
  (void)hipStreamSynchronize(ds->ctx->stream);
  delete ds;
  return NFM_OK;
}

// ------------------------------------------------------------------ model
int32_t nfm_model_create(nfm_ctx* ctx, const nfm_model_cfg* cfg, nfm_model** out) {
  NFM_CHECK(ctx && cfg && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(cfg->kind == NFM_KIND_FM || cfg->kind == NFM_KIND_FFM, NFM_ERR_INVALID, "bad model kind");
  NFM_CHECK(cfg->n_components >= 1, NFM_ERR_INVALID, "nComponents < 1.");
  NFM_CHECK(cfg->n_features >= 1, NFM_ERR_INVALID, "n_features < 1");
  NFM_TRY(use_device(ctx));
  std::unique_ptr<nfm_model> m(new nfm_model());
  m->ctx = ctx;
  m->cfg = *cfg;
  m->k = cfg->n_components;
  m->d = cfg->n_features;
  if (cfg->kind == NFM_KIND_FM) {
    NFM_CHECK(cfg->degree >= 1, NFM_ERR_INVALID, "degree < 1.");
    NFM_CHECK(cfg->fit_lower >= 0 && cfg->fit_lower <= 2, NFM_ERR_INVALID, "bad fit_lower");
    // model/factorization_machine.nim:81-97
    m->n_aug = cfg->fit_lower == NFM_LOWER_AUGMENT ? (cfg->fit_linear ? cfg->degree - 2 : cfg->degree - 1) : 0;
    m->nb = cfg->degree == 1 ? 0 : (cfg->fit_lower == NFM_LOWER_EXPLICIT ? cfg->degree - 1 : 1);
    NFM_CHECK(m->n_aug >= 0, NFM_ERR_INVALID, "fit_lower=augment needs degree >= 2 (fit_linear) or >= 1");
  } else {
    NFM_CHECK(cfg->n_fields >= 1, NFM_ERR_INVALID, "n_fields < 1");
    m->n_aug = 0;
    m->nb = (int)cfg->n_fields;
  }
  m->da = m->d + m->n_aug;
  m->no = m->nb;
  m->kb = m->k;
  if (cfg->kind == NFM_KIND_FM && m->k > 128) {  // wide FM: kc blocks of kb <= 128 factors per order (ModelView::kc)
    m->kc = (m->k + 127) / 128;
    m->kb = (m->k + m->kc - 1) / m->kc;
    m->nb = m->no * m->kc;
  }
  m->L = lanes_for_k(m->kb);
  m->Kp = m->kb <= 128 ? 2 * m->L : ((m->kb + 63) / 64) * 64;  // (field-aware models keep wide rows: the one-sample-in-flight kernel takes them)
  if (m->kb > 128) m->L = 64;
  {
    const size_t bP = pad256(sizeof(double) * std::max<int64_t>(m->nP(), 2)), bw = pad256(sizeof(double) * m->d);
    NFM_TRY(m->arena.alloc(bP + bw + sizeof(double) * SC_COUNT));
    NFM_HIP_CHECK(hipMemsetAsync(m->arena.p, 0, m->arena.bytes, ctx->stream));
    char* base = m->arena.as<char>();
    m->P = {base, bP};
    m->w = {base + bP, bw};
    m->sc = {base + bP + bw, sizeof(double) * SC_COUNT};
  }
  NFM_TRY(m->lams.alloc(sizeof(double) * m->kc * m->Kp));
  double sc[SC_COUNT] = {1.0, 1.0, 0.0, 0, 0, 0, 0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(m->sc.p, sc, sizeof(sc), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  m->uid = register_model(m.get());
  *out = m.release();
  return NFM_OK;
}

int32_t nfm_model_shape(const nfm_model* m, int32_t* n_blocks, int32_t* n_aug) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  if (n_blocks) *n_blocks = m->no;  // the reference's orders (fields): the first extent of its P
  if (n_aug) *n_aug = m->n_aug;
  return NFM_OK;
}

static int not_convex(const nfm_model* m, const char* what) {
  NFM_CHECK(!m->is_cfm(), NFM_ERR_UNSUPPORTED, "%s does not take a ConvexFactorizationMachine%s", what,
            strncmp(what, "nfm_model", 9) == 0 ? " (use nfm_cfm_set_params / nfm_cfm_get_params)" : " (newHazan and newGreedyCD fit it)");
  return NFM_OK;
}

int32_t nfm_model_set_params(nfm_model* m, const double* P, const double* w, double intercept, const double* lams) {
  NFM_CHECK(m && w, NFM_ERR_INVALID, "null argument");
  NFM_TRY(not_convex(m, "nfm_model_set_params"));
  NFM_CHECK(m->nb == 0 || P, NFM_ERR_INVALID, "null P");
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  hipStream_t st = ctx->stream;
  const int64_t n_ref = m->n_ref();
  if (n_ref > 0) {
    DevBuf tmp;
    NFM_TRY(tmp.alloc(sizeof(double) * n_ref));
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.p, P, sizeof(double) * n_ref, hipMemcpyHostToDevice, st));
    if (m->cfg.kind == NFM_KIND_FM)
      NFM_TRY(fm_params_to_device(m, tmp.as<double>(), m->P.as<double>()));
    else
      NFM_TRY(rows_to_device(m, tmp.as<double>(), m->P.as<double>(), 0.0));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  NFM_HIP_CHECK(hipMemcpyAsync(m->w.p, w, sizeof(double) * m->d, hipMemcpyHostToDevice, st));
  double sc[SC_COUNT] = {1.0, 1.0, intercept, 0, 0, 0, 0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(m->sc.p, sc, sizeof(sc), hipMemcpyHostToDevice, st));
  std::vector<double> lp((size_t)m->kc * m->Kp, 0.0);
  for (int s = 0; s < m->k; ++s) lp[(size_t)(s / m->kb) * m->Kp + s % m->kb] = lams ? lams[s] : 1.0;
  NFM_HIP_CHECK(hipMemcpyAsync(m->lams.p, lp.data(), sizeof(double) * lp.size(), hipMemcpyHostToDevice, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  m->initialized = true;
  return NFM_OK;
}

int32_t nfm_model_get_params(nfm_model* m, double* P, double* w, double* intercept) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_TRY(not_convex(m, "nfm_model_get_params"));
  NFM_CHECK(m->initialized, NFM_ERR_NOT_FITTED, "Factorization machines is not fitted.");
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  hipStream_t st = ctx->stream;
  double sc[SC_COUNT];
  NFM_HIP_CHECK(hipMemcpyAsync(sc, m->sc.p, sizeof(sc), hipMemcpyDeviceToHost, st));
  const int64_t n_ref = m->n_ref();
  if (P && n_ref > 0) {
    DevBuf tmp;
    NFM_TRY(tmp.alloc(sizeof(double) * n_ref));
    if (m->cfg.kind == NFM_KIND_FM)
      NFM_TRY(fm_params_from_device(m, m->P.as<double>(), tmp.as<double>(), m->sc.as<double>() + SC_SCALE_P));
    else
      NFM_TRY(rows_from_device(m, m->P.as<double>(), tmp.as<double>(), m->sc.as<double>() + SC_SCALE_P));
    NFM_HIP_CHECK(hipMemcpyAsync(P, tmp.p, sizeof(double) * n_ref, hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (w) NFM_HIP_CHECK(hipMemcpyAsync(w, m->w.p, sizeof(double) * m->d, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  if (w && sc[SC_SCALE_W] != 1.0)
    for (int64_t j = 0; j < m->d; ++j) w[j] *= sc[SC_SCALE_W];
  if (intercept) *intercept = sc[SC_INTERCEPT];
  return NFM_OK;
}

// training needs distinct column ids inside every row (plan.h); decisionFunction / score / metrics do not
static int check_trainable(const nfm_dataset* ds) {
  NFM_CHECK(ds->repeats == 0, NFM_ERR_UNSUPPORTED,
            "%lld repeated column ids inside rows (first in row %lld): the ids of one row must be distinct for training -- merge "
            "repeated entries (decisionFunction, predict and score take the dataset as it is)",
            (long long)ds->repeats, (long long)ds->repeat_row);
  return NFM_OK;
}

static int check_predict_shapes(nfm_model* m, nfm_dataset* ds) {
  NFM_CHECK(m && ds, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(m->ctx == ds->ctx, NFM_ERR_INVALID, "model and dataset belong to different contexts");
  NFM_CHECK(m->initialized, NFM_ERR_NOT_FITTED, "Factorization machines is not fitted.");
  NFM_CHECK(ds->v.d == m->d, NFM_ERR_INVALID, "Invalid nFeatures.");
  if (m->cfg.kind == NFM_KIND_FFM) {
    NFM_CHECK(ds->v.fields != nullptr, NFM_ERR_INVALID, "FFM needs a CSRFieldDataset (fields == NULL)");
    NFM_CHECK(ds->v.n_fields == m->nb, NFM_ERR_INVALID, "Invalid nFields.");
  }
  return NFM_OK;
}

int32_t nfm_decision_function_device(nfm_model* m, nfm_dataset* ds, double* out_dev) {
  NFM_TRY(check_predict_shapes(m, ds));
  NFM_CHECK(out_dev || ds->v.n == 0, NFM_ERR_INVALID, "null out");
  NFM_CHECK(m->cfg.kind == NFM_KIND_FFM || m->cfg.degree <= 6, NFM_ERR_UNSUPPORTED, "degree > 6 unsupported");
  NFM_TRY(use_device(m->ctx));
  if (m->is_cfm()) return launch_cfm_predict(m->ctx, ds->v, m->cfm_view(), out_dev);
  return launch_predict(m->ctx, ds->v, m->view(), out_dev);
}

int32_t nfm_decision_function(nfm_model* m, nfm_dataset* ds, double* out) {
  NFM_TRY(check_predict_shapes(m, ds));
  NFM_CHECK(out || ds->v.n == 0, NFM_ERR_INVALID, "null out");
  NFM_TRY(use_device(m->ctx));
  DevBuf tmp;
  NFM_TRY(tmp.alloc(sizeof(double) * ds->v.n));
  NFM_TRY(nfm_decision_function_device(m, ds, tmp.as<double>()));
  NFM_HIP_CHECK(hipMemcpyAsync(out, tmp.p, sizeof(double) * ds->v.n, hipMemcpyDeviceToHost, m->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return NFM_OK;
}

// score / metrics on the device: decisionFunction stays in HBM, only scalars come back
int32_t nfm_metrics(nfm_model* m, nfm_dataset* ds, double* rmse, double* accuracy, double* rocauc) {
  NFM_TRY(check_predict_shapes(m, ds));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "the dataset has no targets");
  NFM_TRY(use_device(m->ctx));
  DevBuf scores;
  NFM_TRY(scores.alloc(sizeof(double) * std::max<int64_t>(ds->v.n, 1)));
  NFM_TRY(nfm_decision_function_device(m, ds, scores.as<double>()));
  return launch_metrics(m->ctx, ds->v.n, scores.as<double>(), ds->v.y, rmse, accuracy, rocauc);
}

int32_t nfm_score(nfm_model* m, nfm_dataset* ds, double* out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  // model/fm_base.nim:39-48: rmse for regression, accuracy (of signs) for classification
  if (m->cfg.task == NFM_TASK_REGRESSION) return nfm_metrics(m, ds, out, nullptr, nullptr);
  return nfm_metrics(m, ds, nullptr, out, nullptr);
}

// ---- every pair of two row sets (cross.h) ----
// what is refused names the way that remains: one row per pair and decisionFunction
static int check_cross(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, const char* what) {
  NFM_CHECK(m && dsU && dsV, NFM_ERR_INVALID, "null argument");
  static const char* kWay = "materialise the pairs, hstack(U[rep], V[tile]), and call decisionFunction";
  NFM_CHECK(!m->is_cfm(), NFM_ERR_UNSUPPORTED, "%s does not take a ConvexFactorizationMachine: %s", what, kWay);
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED, "%s does not take a field-aware model: %s", what, kWay);
  NFM_CHECK(m->cfg.degree == 2, NFM_ERR_UNSUPPORTED, "%s takes a model of degree 2, not %d: %s", what, (int)m->cfg.degree, kWay);
  NFM_CHECK(!dsU->v.fields && !dsV->v.fields, NFM_ERR_UNSUPPORTED, "%s does not take a field-aware dataset: %s", what, kWay);
  NFM_CHECK(dsU->ctx == dsV->ctx, NFM_ERR_UNSUPPORTED, "%s: U and V belong to different contexts: %s", what, kWay);
  NFM_CHECK(m->ctx == dsU->ctx, NFM_ERR_INVALID, "model and dataset belong to different contexts");
  NFM_CHECK(m->initialized, NFM_ERR_NOT_FITTED, "Factorization machines is not fitted.");
  NFM_CHECK(dsU->v.d + dsV->v.d == m->d, NFM_ERR_INVALID, "Invalid nFeatures.");
  return NFM_OK;
}

int32_t nfm_cross_decision_function_device(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, double* out_dev) {
  NFM_TRY(check_cross(m, dsU, dsV, "crossDecisionFunction"));
  NFM_CHECK(out_dev || dsU->v.n == 0 || dsV->v.n == 0, NFM_ERR_INVALID, "null out");
  NFM_TRY(use_device(m->ctx));
  CrossSides S;
  NFM_TRY(cross_sides(m->ctx, dsU->v, dsV->v, m->view(), &S));
  NFM_TRY(cross_scores(m->ctx, S, 0, S.nU, out_dev));
  NFM_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));  // the sides go back to the block cache: nothing queued may still read them
  return NFM_OK;
}

int32_t nfm_cross_decision_function(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, double* out) {
  NFM_TRY(check_cross(m, dsU, dsV, "crossDecisionFunction"));
  const int64_t nU = dsU->v.n, nV = dsV->v.n;
  NFM_CHECK(out || nU == 0 || nV == 0, NFM_ERR_INVALID, "null out");
  if (nU == 0 || nV == 0) return NFM_OK;
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  size_t mem_free = 0, mem_total = 0;
  NFM_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
  NFM_CHECK((double)nU * (double)nV * 8.0 <= (double)mem_total, NFM_ERR_UNSUPPORTED,
            "crossDecisionFunction: %lld x %lld scores do not fit the device: rank with topK (recommend), or score row slices of U",
            (long long)nU, (long long)nV);
  CrossSides S;
  NFM_TRY(cross_sides(ctx, dsU->v, dsV->v, m->view(), &S));
  // user blocks of whole tiles, about 64 MiB each, leave through the dumps' two pinned buffers while the next one is scored
  int64_t rows = ((int64_t)64 << 20) / (nV * 8) / kCrossTU * kCrossTU;
  rows = std::min(std::max<int64_t>(rows, kCrossTU), nU);
  const int64_t n_pieces = (nU + rows - 1) / rows;
  TextSink sink;
  sink.buf = reinterpret_cast<char*>(out);
  sink.cap = nU * nV * 8;
  DumpPipe P;
  P.ctx = ctx;
  NFM_TRY(P.open(ctx, sink, rows * nV * 8, false));
  for (int64_t p = 0; p < n_pieces; ++p) {
    DumpPipe::Slot& Sl = P.slot[p & 1];
    const int64_t u0 = p * rows, u1 = std::min(nU, u0 + rows);
    NFM_TRY(cross_scores(ctx, S, u0, u1, Sl.out.as<double>()));
    NFM_HIP_CHECK(hipEventRecord(Sl.fmt, ctx->stream));
    NFM_TRY(P.consume(P.slot[(p & 1) ^ 1]));  // block p - 1 leaves while block p is scored
    NFM_HIP_CHECK(hipEventSynchronize(Sl.fmt));
    Sl.len = (u1 - u0) * nV * 8;
    NFM_TRY(P.send(Sl));
  }
  NFM_TRY(P.consume(P.slot[(n_pieces - 1) & 1]));
  return NFM_OK;
}

int32_t nfm_cross_topk(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, int64_t K, int64_t chunk_items, int64_t* ids, double* scores) {
  NFM_TRY(check_cross(m, dsU, dsV, "recommend"));
  const int64_t nU = dsU->v.n, nV = dsV->v.n, most = std::min<int64_t>(nV, kCrossMaxTopK);
  NFM_CHECK(K >= 1 && K <= most, NFM_ERR_INVALID,
            "recommend: topK = %lld is outside 1 .. min(nV, %d) = %lld (crossDecisionFunction returns every score)", (long long)K, kCrossMaxTopK,
            (long long)most);
  NFM_CHECK(chunk_items >= 0, NFM_ERR_INVALID, "recommend: chunkItems < 0");
  NFM_CHECK((ids && scores) || nU == 0, NFM_ERR_INVALID, "null out");
  if (nU == 0) return NFM_OK;
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  CrossSides S;
  NFM_TRY(cross_sides(ctx, dsU->v, dsV->v, m->view(), &S));
  DevBuf ids_dev, scores_dev;
  NFM_TRY(ids_dev.alloc(sizeof(int64_t) * (size_t)(nU * K)));
  NFM_TRY(scores_dev.alloc(sizeof(double) * (size_t)(nU * K)));
  NFM_TRY(cross_topk(ctx, S, K, chunk_items, ids_dev.as<int64_t>(), scores_dev.as<double>()));
  NFM_HIP_CHECK(hipMemcpyAsync(ids, ids_dev.p, sizeof(int64_t) * (size_t)(nU * K), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipMemcpyAsync(scores, scores_dev.p, sizeof(double) * (size_t)(nU * K), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return NFM_OK;
}

int32_t nfm_model_sqnorms(nfm_model* m, double* P_sq, double* w_sq) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_TRY(not_convex(m, "nfm_model_sqnorms"));
  NFM_TRY(use_device(m->ctx));
  DevBuf out;
  NFM_TRY(out.alloc(sizeof(double) * 2));
  NFM_TRY(launch_sqnorms(m->ctx, m->view(), out.as<double>()));
  double h[2];
  NFM_HIP_CHECK(hipMemcpy(h, out.p, sizeof(h), hipMemcpyDeviceToHost));
  if (P_sq) *P_sq = h[0];
  if (w_sq) *w_sq = h[1];
  return NFM_OK;
}

int32_t nfm_model_device_buffers(nfm_model* m, double** P_dev, int64_t* n_P, double** w_dev, int64_t* n_w,
                                 double** scalars_dev, int64_t* n_scalars) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_TRY(not_convex(m, "nfm_model_device_buffers"));
  if (P_dev) *P_dev = m->P.as<double>();
  if (n_P) *n_P = m->nP();
  if (w_dev) *w_dev = m->w.as<double>();
  if (n_w) *n_w = m->d;
  if (scalars_dev) *scalars_dev = m->sc.as<double>();
  if (n_scalars) *n_scalars = SC_COUNT;
  return NFM_OK;
}

int32_t nfm_model_destroy(nfm_model* m) {
  if (!m) return NFM_OK;
  unregister_model(m->uid);
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  delete m;
  return NFM_OK;
}

// ------------------------------------------------------------------ optimizers
static int check_common(nfm_model* m, int loss, int mode, int64_t batch) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_TRY(not_convex(m, "SGD / AdaGrad / MBPSGD"));
  NFM_CHECK(loss >= 0 && loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_CHECK(mode == NFM_MODE_SEQUENTIAL || mode == NFM_MODE_MINIBATCH, NFM_ERR_INVALID, "bad mode");
  NFM_CHECK(mode == NFM_MODE_SEQUENTIAL || batch >= 1, NFM_ERR_INVALID, "batch must be >= 1");
  return NFM_OK;
}

int32_t nfm_sgd_create(nfm_model* m, const nfm_sgd_cfg* c, nfm_opt** out) {
  NFM_CHECK(c && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(check_common(m, c->loss, c->mode, c->batch));
  NFM_CHECK(c->scheduling >= 0 && c->scheduling <= 3, NFM_ERR_INVALID, "bad scheduling id");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_SGD; o->mode = c->mode; o->batch = c->mode == NFM_MODE_MINIBATCH ? c->batch : 1; o->it = 1;
  o->o.eta0 = c->eta0; o->o.alpha0 = c->alpha0; o->o.alpha = c->alpha; o->o.beta = c->beta; o->o.power = c->power;
  o->o.eps = 0.0; o->o.loss_param = c->loss_param; o->o.loss = c->loss; o->o.sched = c->scheduling; o->o.track_viol = 1;
  o->o.touch_cap = 1.0;
  NFM_TRY(use_device(m->ctx));
  NFM_TRY(o->out2.alloc(sizeof(double) * 2));
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_adagrad_create(nfm_model* m, const nfm_adagrad_cfg* c, nfm_opt** out) {
  NFM_CHECK(c && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(check_common(m, c->loss, c->mode, c->batch));
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_ADAGRAD; o->mode = c->mode; o->batch = c->mode == NFM_MODE_MINIBATCH ? c->batch : 1; o->it = 1;
  o->o.eta0 = c->eta0; o->o.alpha0 = c->alpha0; o->o.alpha = c->alpha; o->o.beta = c->beta; o->o.power = 1.0;
  o->o.eps = c->eps; o->o.loss_param = c->loss_param; o->o.loss = c->loss; o->o.sched = 0; o->o.track_viol = c->track_viol;
  o->o.touch_cap = 1.0;
  o->o.ada_cross = 0.0;
  NFM_TRY(use_device(m->ctx));
  NFM_TRY(o->out2.alloc(sizeof(double) * 2));
  {
    const size_t bP = pad256(sizeof(double) * std::max<int64_t>(m->nP(), 2)), bw = pad256(sizeof(double) * m->d);
    NFM_TRY(o->state_arena.alloc(2 * bP + 2 * bw + sizeof(double) * 2));
    NFM_HIP_CHECK(hipMemsetAsync(o->state_arena.p, 0, o->state_arena.bytes, m->ctx->stream));
    char* base = o->state_arena.as<char>();
    o->G = {base, bP};
    o->N = {base + bP, bP};
    o->Gw = {base + 2 * bP, bw};
    o->Nw = {base + 2 * bP + bw, bw};
    o->gsc = {base + 2 * bP + 2 * bw, sizeof(double) * 2};
  }
  o->o.G = o->G.as<double>(); o->o.N = o->N.as<double>(); o->o.Gw = o->Gw.as<double>(); o->o.Nw = o->Nw.as<double>();
  o->o.gsc = o->gsc.as<double>();
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_mbpsgd_create(nfm_model* m, const nfm_mbpsgd_cfg* c, nfm_opt** out) {
  NFM_CHECK(c && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(check_common(m, c->loss, NFM_MODE_MINIBATCH, c->batch));
  NFM_CHECK(c->scheduling >= 0 && c->scheduling <= 3, NFM_ERR_INVALID, "bad scheduling id");
  NFM_CHECK(c->reg >= NFM_REG_L1 && c->reg <= NFM_REG_SQUAREDL21, NFM_ERR_INVALID, "bad regularizer id");
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED, "MBPSGD fits a FactorizationMachine (minibatch_psgd.nim:125-126)");
  NFM_CHECK(m->kc == 1, NFM_ERR_UNSUPPORTED, "MBPSGD supports n_components <= 128 (the matrix prox needs a feature's factors in one row)");
  if (c->reg == NFM_REG_SQUAREDL12)  // squaredl12.nim:103-105
    NFM_CHECK(m->cfg.degree == 2, NFM_ERR_INVALID, "SquaredL12 supports only degree=2.");
  if (c->reg == NFM_REG_SQUAREDL21) {  // squaredl21.nim:27-28
    NFM_CHECK(m->cfg.degree == 2, NFM_ERR_INVALID, "SquaredL21 supports only degree=2.");
    NFM_CHECK(!c->reg_transpose, NFM_ERR_UNSUPPORTED, "SquaredL21 with transpose=true is not supported");
  }
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_PSGD; o->mode = NFM_MODE_MINIBATCH; o->batch = c->batch; o->it = 1;
  o->o.eta0 = c->eta0; o->o.alpha0 = c->alpha0; o->o.alpha = c->alpha; o->o.beta = c->beta; o->o.power = c->power;
  o->o.eps = 0.0; o->o.loss_param = c->loss_param; o->o.loss = c->loss; o->o.sched = c->scheduling; o->o.track_viol = 0;
  o->o.touch_cap = 1.0;
  o->o.gamma = c->gamma; o->o.bsize = (double)c->batch; o->o.reg = c->reg; o->o.reg_transpose = c->reg_transpose ? 1 : 0;
  NFM_TRY(use_device(m->ctx));
  NFM_TRY(o->out2.alloc(sizeof(double) * 2));
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_psgd_create(nfm_model* m, const nfm_mbpsgd_cfg* c, nfm_opt** out) {
  NFM_CHECK(c && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_TRY(not_convex(m, "PSGD"));
  NFM_CHECK(c->loss >= 0 && c->loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_CHECK(c->scheduling >= 0 && c->scheduling <= 3, NFM_ERR_INVALID, "bad scheduling id");
  NFM_CHECK(c->reg >= NFM_REG_L1 && c->reg <= NFM_REG_OMEGACS, NFM_ERR_INVALID, "bad regularizer id");
  NFM_CHECK(c->reg != NFM_REG_SQUAREDL12 && c->reg != NFM_REG_SQUAREDL21, NFM_ERR_UNSUPPORTED,
            "PSGD on the device takes L1 or L21: the step of SquaredL12 / SquaredL21 touches every parameter per sample -- use newMBPSGD "
            "(nfm_mbpsgd_create), which has their proximal operators");
  NFM_CHECK(c->reg != NFM_REG_OMEGATI && c->reg != NFM_REG_OMEGACS, NFM_ERR_UNSUPPORTED,
            "PSGD cannot be used for OmegaTI / OmegaCS: they have no SGD hooks -- use newPCD (OmegaTI) or newPBCD (OmegaCS)");
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED,
            "PSGD fits a FactorizationMachine (psgd.nim:76-78) -- use newSGD or newAdaGrad for a field-aware model");
  NFM_CHECK(m->kc == 1, NFM_ERR_UNSUPPORTED, "PSGD supports n_components <= 128 -- use newMBPSGD's L1 or newSGD for wider models");
  NFM_CHECK(m->cfg.degree <= 6, NFM_ERR_UNSUPPORTED, "PSGD supports degree <= 6 -- use newSGD(mode = sequential) beyond");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_PSGD_SEQ; o->mode = NFM_MODE_SEQUENTIAL; o->batch = 1; o->it = 1;
  o->o.eta0 = c->eta0; o->o.alpha0 = c->alpha0; o->o.alpha = c->alpha; o->o.beta = c->beta; o->o.power = c->power;
  o->o.eps = 0.0; o->o.loss_param = c->loss_param; o->o.loss = c->loss; o->o.sched = c->scheduling; o->o.track_viol = 0;
  o->o.touch_cap = 1.0;
  o->o.gamma = c->gamma; o->o.bsize = 1.0; o->o.reg = c->reg; o->o.reg_transpose = 0;
  NFM_TRY(use_device(m->ctx));
  NFM_TRY(o->out2.alloc(sizeof(double) * 2));
  o->psgd.reset(new PsgdSeqState());
  NFM_TRY(psgd_seq_alloc(m->ctx, m->view(), o->psgd.get()));
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_opt_set_it(nfm_opt* o, int64_t it) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  // newMBPSGD starts at it = 0 and a warm-started fit keeps it (minibatch_psgd.nim:63,153-154)
  NFM_CHECK(it >= (o->kind == OPT_PSGD ? 0 : 1), NFM_ERR_INVALID, "it must be >= 1");
  o->it = it;
  // a new fit starts here: a plan prepared for "the next epoch" of an earlier fit (announced or device-drawn order) is
  // not carried into it
  o->ahead.invalidate();
  o->ahead.offer(nullptr, 0, 0);
  return NFM_OK;
}
int32_t nfm_opt_get_it(nfm_opt* o, int64_t* it) {
  NFM_CHECK(o && it, NFM_ERR_INVALID, "null argument");
  *it = o->it;
  return NFM_OK;
}

// adagrad.nim:52-55: g_sum = 0, g_norm = eps when it == 1
static int adagrad_reset_state(nfm_opt* o) {
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  nfm_ctx* ctx = m->ctx;
  NFM_HIP_CHECK(hipMemsetAsync(o->G.p, 0, o->G.bytes, ctx->stream));
  NFM_HIP_CHECK(hipMemsetAsync(o->Gw.p, 0, o->Gw.bytes, ctx->stream));
  NFM_TRY(launch_fill(ctx, o->N.as<double>(), std::max<int64_t>(m->nP(), 2), o->o.eps));
  NFM_TRY(launch_fill(ctx, o->Nw.as<double>(), m->d, o->o.eps));
  const double g[2] = {0.0, o->o.eps};
  NFM_HIP_CHECK(hipMemcpyAsync(o->gsc.p, g, sizeof(g), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  o->state_ready = true;
  return NFM_OK;
}

int32_t nfm_opt_get_state(nfm_opt* o, double* gsum_P, double* gnorm_P, double* gsum_w, double* gnorm_w, double* gsum_b,
                          double* gnorm_b) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_ADAGRAD, NFM_ERR_INVALID, "only AdaGrad carries state");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  if (!o->state_ready) NFM_TRY(adagrad_reset_state(o));
  const int64_t n_ref = m->n_ref();  // (the state shares the parameters' device layout)
  DevBuf tmp;
  NFM_TRY(tmp.alloc(sizeof(double) * std::max<int64_t>(n_ref, 1)));
  for (int which = 0; which < 2; ++which) {
    double* dst = which ? gnorm_P : gsum_P;
    if (!dst || n_ref == 0) continue;
    NFM_TRY(rows_from_device(m, which ? o->N.as<double>() : o->G.as<double>(), tmp.as<double>(), nullptr));
    NFM_HIP_CHECK(hipMemcpyAsync(dst, tmp.p, sizeof(double) * n_ref, hipMemcpyDeviceToHost, ctx->stream));
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (gsum_w) NFM_HIP_CHECK(hipMemcpyAsync(gsum_w, o->Gw.p, sizeof(double) * m->d, hipMemcpyDeviceToHost, ctx->stream));
  if (gnorm_w) NFM_HIP_CHECK(hipMemcpyAsync(gnorm_w, o->Nw.p, sizeof(double) * m->d, hipMemcpyDeviceToHost, ctx->stream));
  double g[2];
  NFM_HIP_CHECK(hipMemcpyAsync(g, o->gsc.p, sizeof(g), hipMemcpyDeviceToHost, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (gsum_b) *gsum_b = g[0];
  if (gnorm_b) *gnorm_b = g[1];
  return NFM_OK;
}

int32_t nfm_opt_set_state(nfm_opt* o, const double* gsum_P, const double* gnorm_P, const double* gsum_w,
                          const double* gnorm_w, double gsum_b, double gnorm_b) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_ADAGRAD, NFM_ERR_INVALID, "only AdaGrad carries state");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(use_device(ctx));
  const int64_t n_ref = m->n_ref();  // (the state shares the parameters' device layout)
  NFM_CHECK(n_ref == 0 || (gsum_P && gnorm_P), NFM_ERR_INVALID, "null state");
  NFM_CHECK(gsum_w && gnorm_w, NFM_ERR_INVALID, "null state");
  DevBuf tmp;
  NFM_TRY(tmp.alloc(sizeof(double) * std::max<int64_t>(n_ref, 1)));
  if (n_ref > 0) {
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.p, gsum_P, sizeof(double) * n_ref, hipMemcpyHostToDevice, ctx->stream));
    NFM_TRY(rows_to_device(m, tmp.as<double>(), o->G.as<double>(), 0.0));
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    NFM_HIP_CHECK(hipMemcpyAsync(tmp.p, gnorm_P, sizeof(double) * n_ref, hipMemcpyHostToDevice, ctx->stream));
    NFM_TRY(rows_to_device(m, tmp.as<double>(), o->N.as<double>(), o->o.eps));
    NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  NFM_HIP_CHECK(hipMemcpyAsync(o->Gw.p, gsum_w, sizeof(double) * m->d, hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipMemcpyAsync(o->Nw.p, gnorm_w, sizeof(double) * m->d, hipMemcpyHostToDevice, ctx->stream));
  const double g[2] = {gsum_b, gnorm_b};
  NFM_HIP_CHECK(hipMemcpyAsync(o->gsc.p, g, sizeof(g), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  o->state_ready = true;
  return NFM_OK;
}

static int ensure_unit_scale(nfm_model* m) {
  double sc[SC_COUNT];
  NFM_HIP_CHECK(hipMemcpyAsync(sc, m->sc.p, sizeof(sc), hipMemcpyDeviceToHost, m->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  if (sc[SC_SCALE_P] != 1.0 || sc[SC_SCALE_W] != 1.0) {
    ModelView v = m->view();
    v.fit_linear = 1;  // w carries its scale regardless of who trained it
    NFM_TRY(launch_rescale(m->ctx, v));
  }
  return NFM_OK;
}

// what one nfm_opt_epoch call of an optimizer with a group attached exchanges (dp.h)
static int dp_epoch_setup(nfm_opt* o, nfm_model* m, const ModelView& M, DpEpoch* out) {
  NFM_CHECK(o->kind != OPT_PSGD, NFM_ERR_UNSUPPORTED, "MBPSGD has no data-parallel mode");
  DpEpoch& de = *out;
  de.dp = o->dp;
  de.opt_kind = o->kind;
  de.sync_period = o->dp_sync_period;
  de.overlap = o->dp_overlap;
  // SGD: the ranks' increments averaged unless NFM_DP_SUM; AdaGrad: its state increments summed unless NFM_DP_STATE_MEAN
  // (NFM_DP_AUTO, the default no host has to know about: what DESIGN.md section 6 measured as stable at every period --
  // AdaGrad's SUMMED state over-shoots as soon as the ranks run more than one mini-batch between exchanges)
  // AdaGrad, NFM_DP_AUTO (round 5): the summed state when the ranks exchange after every mini-batch (synchronous data-parallel
  // AdaGrad), NFM_DP_STATE_CROSS otherwise -- one rank's progress per epoch at 2 / 4 / 8 ranks for every period, where the averaged
  // state keeps 0.75 of it at 8 ranks and the plain sum diverges (profiles/r05g_dp_convergence.txt)
  const int ada_rule = (o->kind == OPT_ADAGRAD && o->dp_combine == NFM_DP_AUTO) ? (o->dp_sync_period == 1 ? NFM_DP_SUM : NFM_DP_STATE_CROSS) : o->dp_combine;
  const bool averaged = o->kind == OPT_SGD ? o->dp_combine != NFM_DP_SUM : ada_rule == NFM_DP_STATE_MEAN;
  de.combine_w = averaged ? 1.0 / (double)o->dp->t->world : 1.0;
  if (o->kind == OPT_ADAGRAD && o->dp_combine == NFM_DP_STATE_RSQRT) de.combine_w = 1.0 / sqrt((double)o->dp->t->world);  // (SGD: the mean)
  if (o->kind == OPT_SGD) {
    de.arena = m->arena.as<double>();
    de.n = (int64_t)((m->sc.as<char>() - m->arena.as<char>()) / sizeof(double)) + SC_COUNT;
    de.skip_lo = (int64_t)((m->sc.as<char>() - m->arena.as<char>()) / sizeof(double)) + SC_SCALE_P;
    de.skip_hi = de.skip_lo + 2;  // {scale_P, scale_w}
    de.seg_w = (int64_t)((reinterpret_cast<char*>(M.w) - m->arena.as<char>()) / sizeof(double));
    de.seg_sc = (int64_t)((m->sc.as<char>() - m->arena.as<char>()) / sizeof(double));
  } else {
    de.arena = o->state_arena.as<double>();
    de.n = (int64_t)((o->gsc.as<char>() - o->state_arena.as<char>()) / sizeof(double)) + 2;
    if (ada_rule == NFM_DP_STATE_CROSS) {  // (g_sum, g_norm) pairs of P, w and the intercept (dp.h)
      auto off = [&](const Span& sp) { return (int64_t)((sp.as<char>() - o->state_arena.as<char>()) / sizeof(double)); };
      de.combine_w = 1.0;
      static const double gamma = getenv("NFM_DP_CROSS_GAMMA") ? atof(getenv("NFM_DP_CROSS_GAMMA")) : 0.1;
      de.cross_gamma = gamma;
      de.n_pairs = 3;
      de.pair[0][0] = off(o->G); de.pair[0][1] = off(o->N); de.pair[0][2] = std::max<int64_t>(m->nP(), 0);
      de.pair[1][0] = off(o->Gw); de.pair[1][1] = off(o->Nw); de.pair[1][2] = m->d;
      de.pair[2][0] = off(o->gsc); de.pair[2][1] = off(o->gsc) + 1; de.pair[2][2] = 1;
    }
  }
  return NFM_OK;
}


// ------------------------------------------------------------------ the whole-iteration solvers (cd.hip, pbcd.hip, pgd.hip)
// what every entry that takes an optimizer and a dataset starts with: the optimizer's live model, of the dataset's context
static int opt_model(nfm_opt* o, const nfm_dataset* ds, nfm_model** out) {
  NFM_TRY(model_of(o, out));
  NFM_CHECK(ds->ctx == (*out)->ctx, NFM_ERR_INVALID, "optimizer and dataset belong to different contexts");
  return NFM_OK;
}
// ... and a dataset with targets that the model can be trained on (SGD, AdaGrad, MBPSGD)
static int check_training_data(nfm_model* m, nfm_dataset* ds) {
  NFM_TRY(check_predict_shapes(m, ds));
  NFM_TRY(refuse_csc(ds, "a row-wise solver (SGD, AdaGrad, MBPSGD, PSGD)"));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  return check_trainable(ds);
}

// an optimizer of `kind` (made by `maker`), its model and a dataset that fit together, on the model's device
static int whole_iter_check(nfm_opt* o, nfm_dataset* ds, int kind, const char* maker, nfm_model** out) {
  NFM_CHECK(o && ds, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(o->kind == kind, NFM_ERR_INVALID, "not an optimizer made by %s", maker);
  NFM_TRY(opt_model(o, ds, out));
  NFM_TRY(check_predict_shapes(*out, ds));
  if (kind == OPT_PGD) NFM_TRY(refuse_csc(ds, "a full-batch solver (PGD, FISTA, NMAPGD)"));
  if (kind == OPT_KATYUSHA) NFM_TRY(refuse_csc(ds, "Katyusha"));
  NFM_TRY(check_trainable(ds));
  return use_device((*out)->ctx);
}

// the dataset's device pointers and the targets a PGD-family fit was begun on (FISTA's accepted objective and NMAPGD's c
// depend on them)
static uint64_t pgd_data_key(const nfm_dataset* ds) { return ds->serial ^ (ds->y_gen << 32); }

// nfm_opt_epoch of these solvers: the call covers the whole dataset, and the fit was begun on it as it is now
static int whole_iter_range(const nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, bool begun, const char* solver,
                            const char* begin_fn) {
  NFM_CHECK(!perm && begin == 0 && end == ds->v.n, NFM_ERR_INVALID,
            "%s runs whole iterations: perm must be NULL and [begin, end) = [0, nSamples)", solver);
  NFM_CHECK(begun, NFM_ERR_INVALID, "call %s on this dataset (and its current targets) before nfm_opt_epoch", begin_fn);
  return NFM_OK;
}

// one call is one iteration over the whole dataset: cd.nim:156-175 in the reference's feature order, or pgd.nim:186-211 /
// fista.nim:99-135 / nmapgd.nim:221-263
static int32_t whole_iter_epoch(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum,
                                double* viol_sum) {
  nfm_model* m = nullptr;
  if (o->kind == OPT_CD) {
    NFM_TRY(whole_iter_check(o, ds, OPT_CD, "nfm_cd_create", &m));
    const bool begun = o->cd && o->cd->fit_ready && o->cd->fit_uid == ds->uid && o->cd->fit_serial == ds->serial;
    NFM_TRY(whole_iter_range(ds, perm, begin, end, begun, "coordinate descent", "nfm_cd_begin_fit"));
    return cd_epoch(m->ctx, ds->v, m->view(), m->k, o->cdp, o->cd.get(), loss_sum, viol_sum);
  }
  NFM_TRY(whole_iter_check(o, ds, OPT_PGD, "nfm_pgd_create", &m));
  const bool begun = o->pgd->fit_ready && o->pgd->fit_uid == ds->uid && o->pgd->fit_serial == pgd_data_key(ds);
  NFM_TRY(whole_iter_range(ds, perm, begin, end, begun, "a full-batch solver", "nfm_pgd_begin_fit"));
  return pgd_epoch(m->ctx, ds->v, ds->uid, m->view(), o->pgd.get(), loss_sum, viol_sum);
}

// one call is one outer iteration of Katyusha (katyusha.nim:229-262) over the index stream perm[begin .. end)
static int32_t katyusha_epoch(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum,
                              double* viol_sum) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_KATYUSHA, "nfm_katyusha_create", &m));
  KatState* S = o->kat.get();
  const bool begun = S->fit_ready && S->fit_uid == ds->uid && S->fit_serial == pgd_data_key(ds);
  NFM_CHECK(begun, NFM_ERR_INVALID, "call nfm_katyusha_begin_fit on this dataset (and its current targets) before nfm_opt_epoch");
  NFM_CHECK(begin >= 0 && begin <= end, NFM_ERR_INVALID, "bad sample range [%lld,%lld)", (long long)begin, (long long)end);
  NFM_CHECK(end - begin == S->cfg.batch * S->m_inner, NFM_ERR_INVALID,
            "Katyusha: one call is one outer iteration of %lld mini-batches of %lld samples, not %lld samples", (long long)S->m_inner,
            (long long)S->cfg.batch, (long long)(end - begin));
  return kat_epoch(m->ctx, ds->v, ds->uid, m->view(), S, perm, begin, end, loss_sum, viol_sum);
}

// Which regulariser a solver family has a step for, and what an accepted one needs of the model.
enum { FAM_PCD, FAM_PBCD, FAM_PGD };
static int reg_accepted(int family, int reg) {
  static const struct { int family, reg; const char* msg; } refused[] = {
      {FAM_PCD, NFM_REG_L21, "PCD cannot be used for L21."},  // nimfm_sparsefm.nim:124-146: L21 and SquaredL21 have no PCD step
      {FAM_PCD, NFM_REG_SQUAREDL21, "PCD cannot be used for squaredL21."},
      {FAM_PBCD, NFM_REG_SQUAREDL12, "PBCD cannot be used for squaredl12."},  // nimfm_sparsefm.nim:118
      {FAM_PBCD, NFM_REG_OMEGATI, "PBCD cannot be used for OmegaTI (it has no BCD hooks)."},
      {FAM_PGD, NFM_REG_OMEGATI, "OmegaTI has no matrix proximal operator (regularizer/omegati.nim)"},
      {FAM_PCD, NFM_REG_OMEGACS, "PCD cannot be used for OmegaCS (it has no CD hooks)."},  // regularizer/omegacs.nim: BCD hooks only
      {FAM_PGD, NFM_REG_OMEGACS, "OmegaCS has no matrix proximal operator (regularizer/omegacs.nim)"},
  };
  NFM_CHECK(reg >= NFM_REG_L1 && reg <= NFM_REG_OMEGACS, NFM_ERR_INVALID, "bad regularizer id");
  for (const auto& r : refused)
    if (r.family == family && r.reg == reg) return set_error(NFM_ERR_UNSUPPORTED, "%s", r.msg);
  return NFM_OK;
}
// initCD (squaredl12.nim:91-93), initSGD (squaredl12.nim:103-105), initBCD (squaredl21.nim:68-70) and squaredl21.nim:27-28
static int reg_fits_model(int reg, int reg_transpose, const nfm_model* m) {
  if (reg == NFM_REG_SQUAREDL12) NFM_CHECK(m->cfg.degree == 2, NFM_ERR_INVALID, "SquaredL12 supports only degree=2.");
  if (reg == NFM_REG_SQUAREDL21) {
    NFM_CHECK(m->cfg.degree == 2, NFM_ERR_INVALID, "SquaredL21 supports only degree=2.");
    NFM_CHECK(!reg_transpose, NFM_ERR_UNSUPPORTED, "SquaredL21 with transpose=true is not supported");
  }
  return NFM_OK;
}

// what nfm_cd_create refuses, for the creators that have checks of their own to make after it
static int cd_create_check(nfm_model* m, int32_t loss, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(loss >= 0 && loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED, "coordinate descent fits a FactorizationMachine (the reference has none for FFM)");
  NFM_CHECK(m->cfg.degree <= kCdMaxDeg, NFM_ERR_UNSUPPORTED, "coordinate descent: degree > %d unsupported", kCdMaxDeg);
  return NFM_OK;
}

extern "C" {
int32_t nfm_cd_create(nfm_model* m, double alpha0, double alpha, double beta, int32_t loss, double loss_param, nfm_opt** out) {
  NFM_TRY(cd_create_check(m, loss, out));
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_CD; o->mode = NFM_MODE_SEQUENTIAL; o->batch = 1; o->it = 1;
  o->o.alpha0 = alpha0; o->o.alpha = alpha; o->o.beta = beta; o->o.loss = loss; o->o.loss_param = loss_param;
  o->cdp.alpha0 = alpha0; o->cdp.alpha = alpha; o->cdp.beta = beta; o->cdp.loss = loss; o->cdp.loss_param = loss_param;
  o->cd.reset(new CdState());
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_cd_begin_fit(nfm_opt* o, nfm_dataset* ds) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_CD, "nfm_cd_create", &m));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  NFM_TRY(ensure_unit_scale(m));  // CD steps the true parameter values
  return cd_begin_fit(m->ctx, ds->v, ds->uid, ds->serial, m->view(), m->k, o->cdp, o->cd.get());
}

int32_t nfm_cd_schedule(nfm_opt* o, nfm_dataset* ds, int64_t* n_levels, int64_t* widest_level) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_CD, "nfm_cd_create", &m));
  return cd_schedule(m->ctx, ds->v, ds->uid, m->n_aug, o->cd.get(), n_levels, widest_level, o->cdp.chained());
}

// newPCD (pcd.nim:17-35): a CD handle whose P sweeps take a proximal step (cd.hip)
int32_t nfm_pcd_create(nfm_model* m, double alpha0, double alpha, double beta, double gamma, int32_t loss, double loss_param,
                       int32_t reg, int32_t reg_transpose, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(reg_accepted(FAM_PCD, reg));
  NFM_TRY(cd_create_check(m, loss, out));
  NFM_TRY(reg_fits_model(reg, 0, m));
  NFM_TRY(nfm_cd_create(m, alpha0, alpha, beta, loss, loss_param, out));
  nfm_opt* o = *out;
  o->o.gamma = gamma;
  o->cdp.gamma = gamma;
  o->cdp.reg = reg;
  o->cdp.reg_transpose = reg_transpose ? 1 : 0;
  return NFM_OK;
}

// newPBCD (pbcd.nim:20-46): a CD handle whose P sweeps step whole rows (pbcd.hip)
int32_t nfm_pbcd_create(nfm_model* m, double alpha0, double alpha, double beta, double gamma, int32_t loss, double loss_param,
                        int32_t reg, int32_t max_search, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_TRY(reg_accepted(FAM_PBCD, reg));
  // the line search's acceptance test reads a loss total accumulated feature by feature over the whole sweep (pbcd.nim:80-109)
  NFM_CHECK(max_search == 0, NFM_ERR_UNSUPPORTED, "PBCD: maxSearch != 0 (the line search) is not supported");
  NFM_TRY(cd_create_check(m, loss, out));
  NFM_TRY(reg_fits_model(reg, 0, m));
  NFM_TRY(nfm_cd_create(m, alpha0, alpha, beta, loss, loss_param, out));
  nfm_opt* o = *out;
  o->o.gamma = gamma;
  o->cdp.gamma = gamma;
  o->cdp.reg = reg;
  o->cdp.block = true;
  return NFM_OK;
}
}  // extern "C"

// ------------------------------------------------------------------ PGD, FISTA, NMAPGD (pgd.hip)
extern "C" {
int32_t nfm_pgd_create(nfm_model* m, int32_t algo, double alpha0, double alpha, double beta, double gamma, double rho, double sigma,
                       double eta, int32_t loss, double loss_param, int32_t reg, int32_t reg_transpose, int64_t max_search, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  struct { int32_t algo; double alpha0, alpha, beta, gamma, rho, sigma, eta; int32_t loss; double loss_param; int32_t reg, reg_transpose; int64_t max_search; }
      cv{algo, alpha0, alpha, beta, gamma, rho, sigma, eta, loss, loss_param, reg, reg_transpose, max_search}, *c = &cv;
  NFM_CHECK(c->algo >= NFM_PGD_ALGO_PGD && c->algo <= NFM_PGD_ALGO_NMAPGD, NFM_ERR_INVALID, "bad algo id");
  NFM_CHECK(c->loss >= 0 && c->loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_TRY(reg_accepted(FAM_PGD, c->reg));
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED, "PGD, FISTA and NMAPGD fit a FactorizationMachine");
  NFM_CHECK(c->rho > 0.0 && c->rho < 1.0, NFM_ERR_INVALID, "rho must lie in (0, 1): the line search multiplies eta by it");
  NFM_TRY(reg_fits_model(c->reg, c->reg_transpose, m));
  NFM_CHECK(m->kc == 1 || c->reg == NFM_REG_L1, NFM_ERR_UNSUPPORTED,
            "n_components > 128 is supported with L1 only (the other proximal operators need a feature's factors in one row, or a column in one block order)");
  NFM_CHECK(m->no <= 16 && m->cfg.degree <= 6, NFM_ERR_UNSUPPORTED, "degree > 6 unsupported");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_PGD; o->mode = NFM_MODE_SEQUENTIAL; o->batch = 1; o->it = 1;
  o->pgd.reset(new PgdState());
  PgdCfg& p = o->pgd->cfg;
  p.algo = c->algo;
  // newNMAPGD stores alpha0: alpha (nmapgd.nim:44): its alpha0 argument is never read
  p.alpha0 = c->algo == NFM_PGD_ALGO_NMAPGD ? c->alpha : c->alpha0;
  p.alpha = c->alpha; p.beta = c->beta; p.gamma = c->gamma; p.rho = c->rho; p.sigma = c->sigma; p.eta = c->eta;
  p.loss = c->loss; p.loss_param = c->loss_param; p.reg = c->reg; p.reg_transpose = c->reg_transpose ? 1 : 0; p.max_search = c->max_search;
  o->o.alpha0 = p.alpha0; o->o.alpha = p.alpha; o->o.beta = p.beta; o->o.gamma = p.gamma; o->o.loss = p.loss; o->o.loss_param = p.loss_param;
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_pgd_begin_fit(nfm_opt* o, nfm_dataset* ds, int32_t warm_start) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_PGD, "nfm_pgd_create", &m));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  NFM_TRY(ensure_unit_scale(m));  // the solvers step the true parameter values
  return pgd_begin_fit(m->ctx, ds->v, ds->uid, pgd_data_key(ds), m->view(), warm_start != 0, o->pgd.get());
}

int32_t nfm_pgd_last_iter(nfm_opt* o, double* out) {
  NFM_CHECK(o && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(o->kind == OPT_PGD, NFM_ERR_INVALID, "not an optimizer made by nfm_pgd_create");
  const PgdIter& r = o->pgd->last;
  out[NFM_PGD_IT_LOSS] = r.lossVal; out[NFM_PGD_IT_REG] = r.regVal; out[NFM_PGD_IT_VIOL] = r.viol;
  out[NFM_PGD_IT_ETA] = r.eta[0]; out[NFM_PGD_IT_ETA_V] = r.eta[1];
  out[NFM_PGD_IT_TRIALS] = r.trials[0]; out[NFM_PGD_IT_TRIALS_V] = r.trials[1];
  out[NFM_PGD_IT_BRANCH] = r.branch; out[NFM_PGD_IT_T] = r.t; out[NFM_PGD_IT_C] = r.c; out[NFM_PGD_IT_Q] = r.q;
  out[NFM_PGD_IT_START] = r.start[0]; out[NFM_PGD_IT_START_V] = r.start[1];
  return NFM_OK;
}
}  // extern "C"

// ------------------------------------------------------------------ Katyusha (katyusha.hip)
extern "C" {
// newKatyusha (katyusha.nim:24-53)
int32_t nfm_katyusha_create(nfm_model* m, double eta, double alpha0, double alpha, double beta, double gamma, double tau1, double tau2,
                            int32_t loss, double loss_param, int32_t reg, int32_t reg_transpose, int64_t batch, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(loss >= 0 && loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_TRY(reg_accepted(FAM_PGD, reg));
  NFM_CHECK(m->cfg.kind == NFM_KIND_FM, NFM_ERR_UNSUPPORTED, "Katyusha fits a FactorizationMachine");
  NFM_CHECK(eta > 0.0, NFM_ERR_INVALID, "eta must be > 0");
  // coef = (1 - theta) / (1 - theta_pow) (katyusha.nim:150-152) is 0 / 0 when the matching strength is 0
  NFM_CHECK(beta > 0.0, NFM_ERR_INVALID, "beta must be > 0: next_tilde's scale (1 - theta) / (1 - theta^m) is 0 / 0 otherwise");
  NFM_CHECK(alpha > 0.0 || !m->cfg.fit_linear, NFM_ERR_INVALID, "alpha must be > 0 with fitLinear: next_tilde's scale (1 - theta) / (1 - theta^m) is 0 / 0 otherwise");
  NFM_CHECK(alpha0 > 0.0 || !m->cfg.fit_intercept, NFM_ERR_INVALID,
            "alpha0 must be > 0 with fitIntercept: next_tilde's scale (1 - theta) / (1 - theta^m) is 0 / 0 otherwise");
  NFM_CHECK(batch >= 1 && batch <= (int64_t)2147483647, NFM_ERR_INVALID, "miniBatchSize must lie in [1, 2^31-1] (the host resolves miniBatchSize <= 0)");
  NFM_TRY(reg_fits_model(reg, reg_transpose, m));
  NFM_CHECK(m->kc == 1 || reg == NFM_REG_L1, NFM_ERR_UNSUPPORTED,
            "n_components > 128 is supported with L1 only (the other proximal operators need a feature's factors in one row, or a column in one block order)");
  NFM_CHECK(m->no <= 16 && m->cfg.degree <= 6, NFM_ERR_UNSUPPORTED, "degree > 6 unsupported");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_KATYUSHA; o->mode = NFM_MODE_SEQUENTIAL; o->batch = batch; o->it = 1;
  o->kat.reset(new KatState());
  KatCfg& k = o->kat->cfg;
  k.eta = eta; k.alpha0 = alpha0; k.alpha = alpha; k.beta = beta; k.gamma = gamma; k.tau1 = tau1; k.tau2 = tau2;
  k.loss = loss; k.loss_param = loss_param; k.reg = reg; k.reg_transpose = reg_transpose ? 1 : 0; k.batch = batch;
  o->o.alpha0 = alpha0; o->o.alpha = alpha; o->o.beta = beta; o->o.gamma = gamma; o->o.loss = loss; o->o.loss_param = loss_param;
  *out = o.release();
  return NFM_OK;
}

// katyusha.nim:182-219
int32_t nfm_katyusha_begin_fit(nfm_opt* o, nfm_dataset* ds) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_KATYUSHA, "nfm_katyusha_create", &m));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  NFM_TRY(ensure_unit_scale(m));  // the solver steps the true parameter values
  return kat_begin_fit(m->ctx, ds->v, ds->uid, pgd_data_key(ds), m->view(), o->kat.get());
}

// tilde_params (katyusha.nim:250-252 take the verbose line's regVal on it), P in the training layout [nOrders][d + nAugments][k]
int32_t nfm_katyusha_snapshot(nfm_opt* o, double* P, double* w, double* intercept) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_KATYUSHA, NFM_ERR_INVALID, "not an optimizer made by nfm_katyusha_create");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  const KatState* S = o->kat.get();
  NFM_CHECK(S->fit_ready, NFM_ERR_INVALID, "call nfm_katyusha_begin_fit first");
  NFM_TRY(use_device(m->ctx));
  hipStream_t st = m->ctx->stream;
  if (P && m->nP() > 0) {
    DevBuf tmp;
    NFM_TRY(tmp.alloc(sizeof(double) * m->n_ref()));
    NFM_TRY(rows_from_device(m, S->tilde.P(), tmp.as<double>(), nullptr));
    NFM_HIP_CHECK(hipMemcpyAsync(P, tmp.p, sizeof(double) * m->n_ref(), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (w) NFM_HIP_CHECK(hipMemcpyAsync(w, S->tilde.w(), sizeof(double) * m->d, hipMemcpyDeviceToHost, st));
  if (intercept) NFM_HIP_CHECK(hipMemcpyAsync(intercept, S->tilde.sc() + SC_INTERCEPT, sizeof(double), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}
}  // extern "C"

// ------------------------------------------------------------------ ConvexFactorizationMachine and Hazan (cfm.hip)
extern "C" {
// newConvexFactorizationMachine (model/convex_factorization_machine.nim:25-46)
int32_t nfm_cfm_create(nfm_ctx* ctx, int32_t task, int32_t max_components, int32_t fit_intercept, int32_t fit_linear, int32_t ignore_diag,
                       int64_t n_features, nfm_model** out) {
  NFM_CHECK(ctx && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(task == NFM_TASK_REGRESSION || task == NFM_TASK_CLASSIFICATION, NFM_ERR_INVALID, "bad task");
  NFM_CHECK(max_components >= 1, NFM_ERR_INVALID, "maxComponents < 1.");
  NFM_CHECK(n_features >= 1, NFM_ERR_INVALID, "n_features < 1");
  NFM_TRY(use_device(ctx));
  std::unique_ptr<nfm_model> m(new nfm_model());
  m->ctx = ctx;
  m->cfg.kind = NFM_KIND_CFM; m->cfg.task = task; m->cfg.degree = 2; m->cfg.n_components = max_components;
  m->cfg.fit_intercept = fit_intercept ? 1 : 0; m->cfg.fit_linear = fit_linear ? 1 : 0; m->cfg.reserved = ignore_diag ? 1 : 0;
  m->cfg.n_features = n_features;
  m->k = m->kb = max_components;
  m->d = m->da = n_features;
  m->L = 1; m->Kp = 2;  // no factor blocks (nb = 0): the generic views of this handle are never used
  const size_t bP = pad256(sizeof(double) * 2), bw = pad256(sizeof(double) * m->d);
  NFM_TRY(m->arena.alloc(bP + bw + sizeof(double) * SC_COUNT));
  NFM_HIP_CHECK(hipMemsetAsync(m->arena.p, 0, m->arena.bytes, ctx->stream));
  char* base = m->arena.as<char>();
  m->P = {base, bP};
  m->w = {base + bP, bw};
  m->sc = {base + bP + bw, sizeof(double) * SC_COUNT};
  NFM_TRY(m->cfm.alloc(sizeof(double) * ((size_t)m->k * m->d + m->k)));
  NFM_HIP_CHECK(hipMemsetAsync(m->cfm.p, 0, m->cfm.bytes, ctx->stream));
  const double sc[SC_COUNT] = {1.0, 1.0, 0.0, 0, 0, 0, 0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(m->sc.p, sc, sizeof(sc), hipMemcpyHostToDevice, ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  m->uid = register_model(m.get());
  *out = m.release();
  return NFM_OK;
}

int32_t nfm_cfm_set_params(nfm_model* m, int32_t n_components, const double* P, const double* lams, const double* w, double intercept) {
  NFM_CHECK(m && w, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(m->is_cfm(), NFM_ERR_INVALID, "not a model made by nfm_cfm_create");
  NFM_CHECK(n_components >= 0 && n_components <= m->k, NFM_ERR_INVALID, "n_components must lie in [0, maxComponents = %d]", m->k);
  NFM_CHECK(n_components == 0 || (P && lams), NFM_ERR_INVALID, "null P or lams");
  NFM_TRY(use_device(m->ctx));
  hipStream_t st = m->ctx->stream;
  CfmView v = m->cfm_view();
  NFM_HIP_CHECK(hipMemsetAsync(m->cfm.p, 0, m->cfm.bytes, st));
  if (n_components > 0) {
    NFM_HIP_CHECK(hipMemcpyAsync(v.P, P, sizeof(double) * (size_t)n_components * m->d, hipMemcpyHostToDevice, st));
    NFM_HIP_CHECK(hipMemcpyAsync(v.lams, lams, sizeof(double) * n_components, hipMemcpyHostToDevice, st));
  }
  NFM_HIP_CHECK(hipMemcpyAsync(v.w, w, sizeof(double) * m->d, hipMemcpyHostToDevice, st));
  const double sc[SC_COUNT] = {1.0, 1.0, intercept, 0, 0, 0, 0, 0};
  NFM_HIP_CHECK(hipMemcpyAsync(m->sc.p, sc, sizeof(sc), hipMemcpyHostToDevice, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  m->cfm_nc = n_components;
  m->initialized = true;
  return NFM_OK;
}

int32_t nfm_cfm_get_params(nfm_model* m, int32_t* n_components, double* P, double* lams, double* w, double* intercept) {
  NFM_CHECK(m, NFM_ERR_INVALID, "null model");
  NFM_CHECK(m->is_cfm(), NFM_ERR_INVALID, "not a model made by nfm_cfm_create");
  NFM_CHECK(m->initialized, NFM_ERR_NOT_FITTED, "Factorization machines is not fitted.");
  NFM_TRY(use_device(m->ctx));
  hipStream_t st = m->ctx->stream;
  const CfmView v = m->cfm_view();
  const int nc = m->cfm_nc;
  if (n_components) *n_components = nc;
  if (P && nc > 0) NFM_HIP_CHECK(hipMemcpyAsync(P, v.P, sizeof(double) * (size_t)nc * m->d, hipMemcpyDeviceToHost, st));
  if (lams && nc > 0) NFM_HIP_CHECK(hipMemcpyAsync(lams, v.lams, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  if (w) NFM_HIP_CHECK(hipMemcpyAsync(w, v.w, sizeof(double) * m->d, hipMemcpyDeviceToHost, st));
  if (intercept) NFM_HIP_CHECK(hipMemcpyAsync(intercept, v.sc + SC_INTERCEPT, sizeof(double), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

// newHazan (optimizer/hazan.nim:22-46)
int32_t nfm_hazan_create(nfm_model* m, double eta, int64_t max_iter_power, double tol_power, int32_t optimal, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(m->is_cfm(), NFM_ERR_UNSUPPORTED, "Hazan fits a ConvexFactorizationMachine (nfm_cfm_create)");
  NFM_CHECK(max_iter_power >= 0 && max_iter_power <= (int64_t)1 << 40, NFM_ERR_INVALID, "bad maxIterPower");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_HAZAN; o->mode = NFM_MODE_SEQUENTIAL; o->batch = 1; o->it = 1;
  o->hz.reset(new HazanState());
  o->hzc.eta = eta; o->hzc.max_iter_power = max_iter_power; o->hzc.tol_power = tol_power; o->hzc.optimal = optimal ? 1 : 0;
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_hazan_begin_fit(nfm_opt* o, nfm_dataset* ds, double* loss_old) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_HAZAN, "nfm_hazan_create", &m));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  return hazan_begin_fit(m->ctx, ds->v, ds->uid, pgd_data_key(ds), m->cfm_view(), o->hzc, o->hz.get(), loss_old);
}

int32_t nfm_hazan_iter(nfm_opt* o, nfm_dataset* ds, int64_t it, const double* start, double* record) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_HAZAN, "nfm_hazan_create", &m));
  NFM_CHECK(start && record, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(it >= 0, NFM_ERR_INVALID, "it must be >= 0");
  HazanState* S = o->hz.get();
  const bool begun = S->fit_ready && S->fit_uid == ds->uid && S->fit_serial == pgd_data_key(ds);
  NFM_CHECK(begun, NFM_ERR_INVALID, "call nfm_hazan_begin_fit on this dataset (and its current targets) before nfm_hazan_iter");
  int32_t nc = m->cfm_nc;
  const int rc = hazan_iter(m->ctx, ds->v, m->cfm_view(), o->hzc, S, it, start, &nc, record);
  if (rc != NFM_OK) {
    S->fit_ready = false;  // the resident state is half-way through an iteration
    return rc;
  }
  m->cfm_nc = nc;
  return NFM_OK;
}

// newGreedyCD (optimizer/greedy_cd.nim:25-30)
int32_t nfm_gcd_create(nfm_model* m, double alpha0, double alpha, double beta, int32_t loss, double loss_param, int64_t max_iter_power,
                       double tol_power, int32_t refit_fully, nfm_opt** out) {
  NFM_CHECK(m && out, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(m->is_cfm(), NFM_ERR_UNSUPPORTED, "GreedyCD fits a ConvexFactorizationMachine (nfm_cfm_create)");
  NFM_CHECK(loss >= 0 && loss <= 3, NFM_ERR_INVALID, "bad loss id");
  NFM_CHECK(max_iter_power >= 0 && max_iter_power <= (int64_t)1 << 40, NFM_ERR_INVALID, "bad maxIterPower");
  std::unique_ptr<nfm_opt> o(new nfm_opt());
  o->ctx = m->ctx; o->m = m; o->m_uid = m->uid; o->kind = OPT_GCD; o->mode = NFM_MODE_SEQUENTIAL; o->batch = 1; o->it = 1;
  o->gcd.reset(new GcdState());
  o->gcdc.alpha0 = alpha0; o->gcdc.alpha = alpha; o->gcdc.beta = beta; o->gcdc.loss = loss; o->gcdc.loss_param = loss_param;
  o->gcdc.max_iter_power = max_iter_power; o->gcdc.tol_power = tol_power; o->gcdc.refit_fully = refit_fully ? 1 : 0;
  *out = o.release();
  return NFM_OK;
}

int32_t nfm_gcd_begin_fit(nfm_opt* o, nfm_dataset* ds, double* loss_old, double* reg_old) {
  nfm_model* m = nullptr;
  NFM_TRY(whole_iter_check(o, ds, OPT_GCD, "nfm_gcd_create", &m));
  NFM_CHECK(ds->has_y, NFM_ERR_INVALID, "dataset has no targets");
  return gcd_begin_fit(m->ctx, ds->v, ds->uid, pgd_data_key(ds), m->cfm_view(), o->gcdc, o->gcd.get(), loss_old, reg_old);
}

// a GreedyCD step on the dataset the fit was begun on; a failed step leaves the resident state half-way: the fit ends
static int gcd_step_check(nfm_opt* o, nfm_dataset* ds, nfm_model** m, const char* fn) {
  NFM_TRY(whole_iter_check(o, ds, OPT_GCD, "nfm_gcd_create", m));
  const HazanState& H = o->gcd->core;
  const bool begun = H.fit_ready && H.fit_uid == ds->uid && H.fit_serial == pgd_data_key(ds);
  NFM_CHECK(begun, NFM_ERR_INVALID, "call nfm_gcd_begin_fit on this dataset (and its current targets) before %s", fn);
  return NFM_OK;
}

int32_t nfm_gcd_outer_begin(nfm_opt* o, nfm_dataset* ds, double* record) {
  nfm_model* m = nullptr;
  NFM_TRY(gcd_step_check(o, ds, &m, "nfm_gcd_outer_begin"));
  NFM_CHECK(record, NFM_ERR_INVALID, "null argument");
  GcdState* S = o->gcd.get();
  NFM_CHECK(!S->outer_open, NFM_ERR_INVALID, "nfm_gcd_outer_begin: the previous outer iteration was not closed by nfm_gcd_outer_end");
  const int rc = gcd_outer_begin(m->ctx, ds->v, m->cfm_view(), o->gcdc, S, record);
  if (rc != NFM_OK) {
    S->core.fit_ready = false;
    return rc;
  }
  S->outer_open = true;
  return NFM_OK;
}

int32_t nfm_gcd_inner(nfm_opt* o, nfm_dataset* ds, const double* start, int32_t refit, double* record) {
  nfm_model* m = nullptr;
  NFM_TRY(gcd_step_check(o, ds, &m, "nfm_gcd_inner"));
  NFM_CHECK(record, NFM_ERR_INVALID, "null argument");
  GcdState* S = o->gcd.get();
  NFM_CHECK(S->outer_open, NFM_ERR_INVALID, "call nfm_gcd_outer_begin before nfm_gcd_inner");
  // greedy_cd.nim:350: a base is added exactly while fewer than maxComponents lams are non-zero (then a free slot exists)
  NFM_CHECK((start != nullptr) == (S->nc_nonzero < m->k), NFM_ERR_INVALID,
            "nfm_gcd_inner takes a start vector exactly when nComponents (%d) < maxComponents (%d)", S->nc_nonzero, m->k);
  int32_t nc = m->cfm_nc;
  const int rc = gcd_inner(m->ctx, ds->v, m->cfm_view(), o->gcdc, S, start, refit ? 1 : 0, &nc, record);
  if (rc != NFM_OK) {
    S->core.fit_ready = false;
    return rc;
  }
  m->cfm_nc = nc;
  return NFM_OK;
}

int32_t nfm_gcd_outer_end(nfm_opt* o, nfm_dataset* ds, int32_t recompute, double* loss, double* reg) {
  nfm_model* m = nullptr;
  NFM_TRY(gcd_step_check(o, ds, &m, "nfm_gcd_outer_end"));
  GcdState* S = o->gcd.get();
  NFM_CHECK(S->outer_open, NFM_ERR_INVALID, "call nfm_gcd_outer_begin before nfm_gcd_outer_end");
  const int rc = gcd_outer_end(m->ctx, ds->v, m->cfm_view(), o->gcdc, S, recompute ? 1 : 0, loss, reg);
  if (rc != NFM_OK) {
    S->core.fit_ready = false;
    return rc;
  }
  S->outer_open = false;
  return NFM_OK;
}
}  // extern "C"

static int32_t opt_epoch_range(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum,
                               double* viol_sum);

// the entries one epoch call may hold (the plan's touch tables and the window's dependency table index them with 32 bits)
static int64_t max_epoch_nnz() {
  int64_t cap = (int64_t)2147483647;
#ifdef NFM_TEST_HOOKS  // (libnimfm_hip_testhooks.so only: lets a test cut a small epoch into pieces)
  if (const char* env = getenv("NFM_TEST_MAX_EPOCH_NNZ")) cap = atoll(env);
#endif
  return cap;
}

// ---- what the epoch entries share: the range check (wraps: MBPSGD's index stream may pass the end of the data,
// minibatch_psgd.nim:104-108), the host-side check of an order's ids, its upload ----
static int check_sample_range(const nfm_dataset* ds, int64_t begin, int64_t end, bool wraps = false) {
  NFM_CHECK(begin >= 0 && begin <= end && (end <= ds->v.n || wraps), NFM_ERR_INVALID, "bad sample range [%lld,%lld)", (long long)begin, (long long)end);
  return NFM_OK;
}
static int check_perm_ids(const nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end) {
  if (perm)
    for (int64_t p = begin; p < end; ++p)
      NFM_CHECK(perm[p] >= 0 && perm[p] < ds->v.n, NFM_ERR_INVALID, "perm[%lld] = %lld out of range", (long long)p, (long long)perm[p]);
  return NFM_OK;
}
// perm[begin .. end) into o->perm_dev; *perm_dev is indexed by ABSOLUTE position (null: no order given, the dataset's own)
static int upload_perm(nfm_opt* o, hipStream_t st, const int64_t* perm, int64_t begin, int64_t end, const int64_t** perm_dev) {
  *perm_dev = nullptr;
  if (!perm) return NFM_OK;
  NFM_TRY(o->perm_dev.ensure(sizeof(int64_t) * (end - begin)));
  NFM_HIP_CHECK(hipMemcpyAsync(o->perm_dev.p, perm + begin, sizeof(int64_t) * (end - begin), hipMemcpyHostToDevice, st));
  *perm_dev = o->perm_dev.as<int64_t>() - begin;
  return NFM_OK;
}

// ---- PSGD (optimizer/psgd.nim): begin_fit, the range call and finalize ----
static int psgd_seq_check(nfm_opt* o, nfm_dataset* ds, nfm_model** m) {
  NFM_CHECK(o && ds, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(o->kind == OPT_PSGD_SEQ, NFM_ERR_INVALID, "not an optimizer made by nfm_psgd_create");
  NFM_TRY(opt_model(o, ds, m));
  NFM_TRY(check_training_data(*m, ds));
  return use_device((*m)->ctx);
}

int32_t nfm_psgd_begin_fit(nfm_opt* o, nfm_dataset* ds) {
  nfm_model* m = nullptr;
  NFM_TRY(psgd_seq_check(o, ds, &m));
  NFM_TRY(ensure_unit_scale(m));  // the stored P and w are the working values: a model SGD left scaled is multiplied out first
  PsgdSeqState* S = o->psgd.get();
  S->fit_ready = false;
  NFM_TRY(psgd_seq_begin_fit(m->ctx, m->view(), S));
  S->fit_ready = true;
  S->fit_uid = ds->uid;
  S->fit_serial = ds->serial;
  return NFM_OK;
}

static int32_t psgd_seq_epoch(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum, double* viol_sum) {
  nfm_model* m = nullptr;
  NFM_TRY(psgd_seq_check(o, ds, &m));
  PsgdSeqState* S = o->psgd.get();
  NFM_CHECK(S->fit_ready && S->fit_uid == ds->uid && S->fit_serial == ds->serial, NFM_ERR_INVALID,
            "call nfm_psgd_begin_fit on this dataset before nfm_opt_epoch");
  NFM_TRY(check_sample_range(ds, begin, end));
  NFM_CHECK(!o->dp, NFM_ERR_UNSUPPORTED, "PSGD has no data-parallel mode");
  nfm_ctx* ctx = m->ctx;
  const int64_t ns = end - begin;
  double ls = 0.0;
  if (ns > 0) {
    const int64_t* perm_dev = nullptr;
    NFM_TRY(check_perm_ids(ds, perm, begin, end));
    NFM_TRY(upload_perm(o, ctx->stream, perm, begin, end, &perm_dev));
    NFM_TRY(psgd_seq_run(ctx, ds->v, m->view(), o->o, S, perm_dev, begin, end, o->it, ds->max_row + m->n_aug, &ls));
    o->it += ns;
  }
  if (loss_sum) *loss_sum = ls;
  if (viol_sum) *viol_sum = 0.0;  // the solver has none (psgd.nim:198)
  return NFM_OK;
}

int32_t nfm_psgd_finalize(nfm_opt* o) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_PSGD_SEQ, NFM_ERR_INVALID, "not an optimizer made by nfm_psgd_create");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  NFM_TRY(use_device(m->ctx));
  NFM_CHECK(o->psgd->fit_ready, NFM_ERR_INVALID, "call nfm_psgd_begin_fit before nfm_psgd_finalize");
  return psgd_seq_finalize(m->ctx, m->view(), o->o, o->psgd.get());
}

int32_t nfm_opt_epoch(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum,
                      double* viol_sum) {
  NFM_CHECK(o && ds, NFM_ERR_INVALID, "null argument");
  if (o->kind == OPT_PSGD_SEQ) return psgd_seq_epoch(o, ds, perm, begin, end, loss_sum, viol_sum);
  if (o->kind == OPT_CD || o->kind == OPT_PGD) return whole_iter_epoch(o, ds, perm, begin, end, loss_sum, viol_sum);
  if (o->kind == OPT_KATYUSHA) return katyusha_epoch(o, ds, perm, begin, end, loss_sum, viol_sum);
  NFM_CHECK(o->kind != OPT_HAZAN, NFM_ERR_INVALID, "Hazan's outer iteration is nfm_hazan_iter (it takes the power method's start vector)");
  NFM_CHECK(o->kind != OPT_GCD, NFM_ERR_INVALID, "GreedyCD's steps are nfm_gcd_outer_begin / nfm_gcd_inner / nfm_gcd_outer_end");
  // A range of more than 2^31 - 1 entries (288 GB hold datasets several times that) is walked as consecutive pieces: an epoch
  // call IS the sequence of its sub-range calls (sequential mode: any cut; mini-batch mode: cuts at mini-batch boundaries --
  // tests/test_gpu_fullsize.py holds one call against two), so the results are those of the one call.  The bound on a piece's
  // entries is samples x the longest row.  Not with a data-parallel group (the exchange points are laid out per call), and a
  // device-drawn order (nfm_opt_set_shuffle) then shuffles inside each piece.
  const int64_t row_max = std::max<int64_t>((int64_t)ds->max_row + 8, 1), cap = max_epoch_nnz();
  const int64_t ns_all = end - begin;
  // (an order over distinct samples holds no more entries than the dataset, however long its longest row is: one outlier row
  // must not cut every epoch of a small dataset into pieces.  MBPSGD's index stream may wrap, so only the product bounds it.)
  bool may_exceed = ns_all > cap / row_max;
  if (may_exceed && o->kind != OPT_PSGD && ns_all <= ds->v.n && ds->v.nnz + 8 * ns_all <= cap) may_exceed = false;
  if (begin >= 0 && ns_all > 0 && !o->dp && may_exceed && (perm || end <= ds->v.n)) {
    const int64_t B = o->mode == NFM_MODE_MINIBATCH ? std::max<int64_t>(o->batch, 1) : 1;
    int64_t piece = cap / row_max / B * B;  // whole mini-batches
    NFM_CHECK(piece >= B, NFM_ERR_UNSUPPORTED, "one mini-batch of %lld samples may hold more than 2^31-1 entries (longest row %lld)",
              (long long)B, (long long)row_max);
    double ls = 0.0, vs = 0.0;
    for (int64_t p0 = begin; p0 < end;) {
      // AdaGrad's very first step is a mini-batch of its own (adagrad.nim:171): the piece that holds it is one sample longer
      const int64_t lead = (o->mode == NFM_MODE_MINIBATCH && o->kind == OPT_ADAGRAD && o->it == 1) ? 1 : 0;
      const int64_t p1 = std::min(end, p0 + piece - (lead ? B - 1 : 0));
      double l1 = 0.0, v1 = 0.0;
      NFM_TRY(opt_epoch_range(o, ds, perm, p0, p1, &l1, &v1));
      ls += l1;
      vs += v1;
      p0 = p1;
    }
    if (loss_sum) *loss_sum = ls;
    if (viol_sum) *viol_sum = vs;
    return NFM_OK;
  }
  return opt_epoch_range(o, ds, perm, begin, end, loss_sum, viol_sum);
}

// ---- one epoch call of SGD, AdaGrad or MBPSGD over [begin, end), in named steps ----
// the call checks, in the order their messages have been reported in since there has been more than one
static int epoch_call_check(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, nfm_model** out) {
  NFM_CHECK(o && ds, NFM_ERR_INVALID, "null argument");
  NFM_TRY(opt_model(o, ds, out));
  NFM_CHECK(!o->dp || dp_is_live(o->dp, o->dp_uid), NFM_ERR_INVALID,
            "the optimizer's data-parallel group was destroyed; detach it (nfm_opt_set_dp(o, NULL, 0, 0)) or attach a new one");
  NFM_TRY(check_training_data(*out, ds));
  NFM_TRY(check_sample_range(ds, begin, end, /*wraps=*/o->kind == OPT_PSGD && perm));
  if (o->kind == OPT_PSGD)
    NFM_CHECK((end - begin) % o->batch == 0, NFM_ERR_INVALID, "MBPSGD: %lld samples are not a whole number of mini-batches of %lld",
              (long long)(end - begin), (long long)o->batch);
  if (o->mode == NFM_MODE_SEQUENTIAL) NFM_TRY(check_perm_ids(ds, perm, begin, end));  // mini-batch mode checks the ids on the device (plan.hip)
  return use_device((*out)->ctx);
}

// -- NFM_MODE_SEQUENTIAL --
// The window kernel's workgroups wait for each other; should one of those waits time out (CUs held by another tenant)
// the call's samples are partly applied.  So the call starts from a snapshot of everything it may write -- the model's
// arena, AdaGrad's state arena behind it: one device-to-device copy, 0.2 ms for the headline's 520 MB -- and an aborted
// call is put back and run by the one-workgroup kernel.
static size_t seq_snapshot_bytes(const nfm_opt* o, const nfm_model* m) { return m->arena.bytes + (o->kind == OPT_ADAGRAD ? o->state_arena.bytes : 0); }
static int seq_snapshot(nfm_opt* o, nfm_model* m, bool restore) {
  char* snap = o->seqwin->snap.as<char>();
  DevBuf* const arenas[2] = {&m->arena, o->kind == OPT_ADAGRAD ? &o->state_arena : nullptr};
  for (DevBuf* a : arenas) {
    if (!a) continue;
    NFM_HIP_CHECK(hipMemcpyAsync(restore ? a->p : snap, restore ? snap : a->p, a->bytes, hipMemcpyDeviceToDevice, m->ctx->stream));
    snap += a->bytes;
  }
  return NFM_OK;
}

// The call is offered the window (win_route, seq_route.h); what is left needs the device: there must be memory for the snapshot
// (then it is allocated on return).
static bool seq_window_offered(nfm_opt* o, nfm_model* m, const WinRoute& R, size_t snap_bytes) {
  nfm_ctx* ctx = m->ctx;
  if (o->seqwin && o->seqwin->fallbacks >= 2) o->seqwin->snap.release();  // (no more window launches from this optimizer: its snapshot goes back)
  if (!R.offered) return false;
  if (!o->seqwin) o->seqwin.reset(new SeqWin());
  // A model (+ AdaGrad state) beyond half of the free memory has no room for its snapshot: that fit runs in the
  // one-workgroup kernel, which needs none -- it must not fail for want of a safety copy.
  bool have_snap = o->seqwin->snap.ensure(snap_bytes) == NFM_OK;
#ifdef NFM_TEST_HOOKS  // (libnimfm_hip_testhooks.so only)
  if (getenv("NFM_TEST_NO_SNAPSHOT") && atoi(getenv("NFM_TEST_NO_SNAPSHOT")) != 0) {
    o->seqwin->snap.release();
    have_snap = false;
  }
#endif
  if (!have_snap) {
    (void)hipGetLastError();  // (the failed allocation's sticky error)
    ctx->timing.acc["seq_window_no_snapshot"].launches += 1;
  }
  return have_snap;
}

// the window launch from a snapshot; *windowed: the call is done (false: the launch aborted and everything is put back)
static int seq_window_epoch(nfm_opt* o, nfm_model* m, nfm_dataset* ds, const ModelView& Mw, const WinRoute& R, const SeqKnobs& K,
                            const int64_t* perm_dev, bool has_perm, int64_t begin, int64_t end, bool* windowed) {
  nfm_ctx* ctx = m->ctx;
  SeqWin* sw = o->seqwin.get();
  NFM_TRY(seq_snapshot(o, m, /*restore=*/false));
  const int rc = launch_sequential_window(ctx, o->kind, ds->v, Mw, o->o, perm_dev, begin, end, o->it, R, K, o->out2.as<double>(), sw,
                                          (ds->uid << 20) ^ ds->serial, has_perm);
  if (rc == NFM_WIN_FALLBACK) {
    NFM_TRY(seq_snapshot(o, m, /*restore=*/true));
    ++sw->fallbacks;
    sw->clean_calls = 0;
    ctx->timing.acc["seq_window_fallback"].launches += 1;  // counted (timing on or off) where tests and bench.py see it: nfm_ctx_timing_get
    return NFM_OK;
  }
  NFM_TRY(rc);
  *windowed = true;
  if (sw->fallbacks > 0 && ++sw->clean_calls >= 16) {  // (a tenant that held CUs once is not held against the optimizer for ever)
    --sw->fallbacks;
    sw->clean_calls = 0;
  }
  return NFM_OK;
}

static int seq_epoch(nfm_opt* o, nfm_model* m, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* out2) {
  nfm_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const int64_t ns = end - begin;
  const ModelView M = m->view();
  NFM_CHECK(!o->dp, NFM_ERR_UNSUPPORTED, "the data-parallel exchange needs NFM_MODE_MINIBATCH");
  const int64_t* perm_dev = nullptr;
  NFM_TRY(upload_perm(o, st, perm, begin, end, &perm_dev));
  bool windowed = false;
  // which kernels the call takes is decided here, once (seq_route.h)
  const SeqKnobs K = seq_knobs();
  const int m_cap = ds->max_row + m->n_aug;
  const size_t snap_bytes = seq_snapshot_bytes(o, m);
  const WinRoute R = win_route(seq_shape(M, m_cap, ns, ds->v.nnz, o->kind == OPT_ADAGRAD, ctx->n_cu), K, o->seqwin ? o->seqwin->fallbacks : 0, snap_bytes);
  if (seq_window_offered(o, m, R, snap_bytes))  // (65 ... 128 factors: the table read as two blocks of 64)
    NFM_TRY(seq_window_epoch(o, m, ds, seq_window_view(M, R), R, K, perm_dev, perm != nullptr, begin, end, &windowed));
  if (!windowed)
    NFM_TRY(launch_sequential(ctx, o->kind, ds->v, seq_row_view(M), o->o, perm_dev, begin, end, o->it, m_cap, o->out2.as<double>(), K));
  NFM_HIP_CHECK(hipMemcpyAsync(out2, o->out2.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  return NFM_OK;
}

// -- NFM_MODE_MINIBATCH --
struct MbCall {  // one mini-batch call: what its plan is keyed by and built with
  nfm_opt* o;
  nfm_model* m;
  nfm_dataset* ds;
  const int64_t* perm;
  PlanKey key;
  bool want_tq, sort_by_count;
  bool dev_shuffle;  // the order is the device's draw of (shuffle_seed, shuffle_epoch)
  int64_t ns() const { return key.end - key.begin; }
};
static MbCall mb_call(nfm_opt* o, nfm_model* m, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end) {
  // Features touched once per batch are updated by the row phase itself ("singles"); worth the
  // second visit of the row only when they are a sizeable share of the touches.  With a touch
  // rate lambda = batch * nnz_per_row / d per feature that share is about exp(-lambda).
  const double lambda = (double)o->batch * ((double)ds->v.nnz / (double)std::max<int64_t>(ds->v.n, 1)) / (double)m->d;
  bool use_singles = o->kind != OPT_PSGD && m->cfg.kind == NFM_KIND_FM && m->cfg.degree == 2 && m->nb == 1 && (o->batch == 1 || lambda <= 1.4);
  if (const char* env = getenv("NFM_SINGLES")) use_singles = use_singles && atoi(env) != 0;  // tuning override
  bool sort_by_count = m->Kp * (int)sizeof(double) >= 128;  // rows of at least one 128-byte line (plan.hip)
  if (const char* env = getenv("NFM_SORT_BY_COUNT")) sort_by_count = atoi(env) != 0;  // tuning override
  const bool first_singleton = o->kind == OPT_ADAGRAD && o->it == 1;
  return MbCall{o, m, ds, perm, PlanKey{ds->uid, ds->v.nnz, begin, end, o->batch, first_singleton, m->n_aug, use_singles},
                /*want_tq=*/m->cfg.kind == NFM_KIND_FFM, sort_by_count, /*dev_shuffle=*/!perm && o->shuffle_seed >= 0 && o->kind != OPT_PSGD};
}

// o->plan becomes the plan of the call: the one built beside the previous call if it is this call's, the last call's if the
// call repeats it in the dataset's own order, else one built now.  Which of the three is counted, timing enabled or not.
static int mb_obtain_plan(const MbCall& c) {
  nfm_opt* o = c.o;
  nfm_ctx* ctx = c.m->ctx;
  PlanAhead& A = o->ahead;
  const char* path = "plan_path_built";
  if ((c.dev_shuffle || c.perm) && A.matches(c.key, c.perm, o->shuffle_epoch)) {
    std::swap(o->plan, A.plan);
    if (c.dev_shuffle) o->perm_gen.take(A.order);
    A.invalidate();
    path = "plan_path_ahead_taken";
  } else if (!c.dev_shuffle && !c.perm && o->plan && !o->plan->has_perm && plan_is(*o->plan, c.key)) {
    path = "plan_path_reused";  // (a plan built ahead stays ready)
  } else {
    if (!o->plan) o->plan.reset(new Plan());
    TimedLaunch tl(ctx, "plan_build");
    if (c.dev_shuffle) {
      NFM_TRY(gen_permutation(ctx, ctx->stream, o->shuffle_seed, o->shuffle_epoch, c.key.begin, c.ns(), &o->perm_gen));
      const FeistelKey fk = feistel_key(o->shuffle_seed, o->shuffle_epoch, c.key.begin, c.ns());  // (the order as a function: plan.h)
      NFM_TRY(build_plan(ctx, c.ds, c.key, c.want_tq, c.sort_by_count, o->plan.get(), nullptr, ctx->stream, o->perm_gen.as<int64_t>(), &c.ds->csc, &fk));
    } else {
      NFM_TRY(build_plan(ctx, c.ds, c.key, c.want_tq, c.sort_by_count, o->plan.get(), c.perm, nullptr, nullptr, c.perm ? &c.ds->csc : nullptr));
    }
    A.invalidate();
  }
  ctx->timing.acc[path].launches += 1;
  return NFM_OK;
}

// The plan of the NEXT call, enqueued on the plan stream (its host-side waits block on that stream only) while this call's
// epoch runs: of the announced array, or of the order the device draws next.  A fit's first step is behind it by then.
static int mb_build_ahead(const MbCall& c, const int64_t* announced) {
  nfm_opt* o = c.o;
  nfm_ctx* ctx = c.m->ctx;
  PlanAhead& A = o->ahead;
  PlanKey next = c.key;
  next.first_singleton = false;
  A.invalidate();  // (the build writes over the plan it holds)
  if (!A.plan) A.plan.reset(new Plan());
  if (announced) {
    NFM_TRY(build_plan(ctx, c.ds, next, c.want_tq, c.sort_by_count, A.plan.get(), announced, A.stream, nullptr, &c.ds->csc));
  } else {
    NFM_TRY(gen_permutation(ctx, A.stream, o->shuffle_seed, o->shuffle_epoch + 1, next.begin, c.ns(), &A.order));
    const FeistelKey fk = feistel_key(o->shuffle_seed, o->shuffle_epoch + 1, next.begin, c.ns());
    NFM_TRY(build_plan(ctx, c.ds, next, c.want_tq, c.sort_by_count, A.plan.get(), nullptr, A.stream, A.order.as<int64_t>(), &c.ds->csc, &fk));
  }
  A.mark_ready(next, announced, o->shuffle_epoch + 1);
  ctx->timing.acc["plan_ahead_built"].launches += 1;
  return NFM_OK;
}

// The ranks of a group run the call together on their own shards (equal step counters at its start): the exchange points
// of the call are agreed on, and the hooks that serve them are set on o->W.  They refer to *de.
static int dp_epoch_open(nfm_opt* o, nfm_model* m, const ModelView& M, DpEpoch* de) {
  NFM_TRY(dp_epoch_setup(o, m, M, de));
  // leading mini-batches of the regular length (everything but a shorter tail) look alike on every rank
  const Plan& PL = *o->plan;
  int64_t regular = PL.n_batches;
  if (PL.n_batches > 0 && PL.bat_pos[PL.n_batches] - PL.bat_pos[PL.n_batches - 1] < o->batch && !(PL.first_singleton && PL.n_batches == 1))
    regular = PL.n_batches - 1;
  NFM_TRY(dp_epoch_begin(*de, regular, PL.n_batches));
  o->W.after_batch = [de](int64_t b) { return dp_after_batch(*de, b); };
  o->W.is_sync = nullptr;  // (no graphs for the threads of a local group: dp.h)
  if (!o->dp->t->in_process)
    o->W.is_sync = [de](int64_t b) { return de->sync_period > 0 && (b + 1) % de->sync_period == 0 && (b + 1) / de->sync_period <= de->n_sync; };
  o->W.seg_key_now = (de->sync_period << 32) + de->n_sync;
  return NFM_OK;
}
// The hooks refer to the caller's frame: whatever way the call leaves, they are taken off again; a call that fails between
// a sync point and its fold-in leaves no exchange marked pending (dp_epoch_begin would refuse every later epoch).
struct DpHooksGuard {
  nfm_opt* o;
  bool ok = false;
  ~DpHooksGuard() {
    o->W.after_batch = nullptr;
    o->W.is_sync = nullptr;
    if (!ok && o->dp) {
      // the all-reduce of the last sync point may still be running on the group's stream (it reads dp->snap and
      // writes dp->recv): the next epoch must not overwrite them under it
      if (o->dp->pending && o->dp->comm) (void)hipStreamSynchronize(o->dp->comm);
      o->dp->pending = false;
    }
  }
};
// The closing exchange: out2 = this rank's loss / viol sums over its ns samples (an empty shard: zeros) becomes the group's.
// The reference's threads share ONE step counter (sgd_multi.nim:37): o->it advances by the samples of the OTHER ranks here,
// by this rank's own in the tail of the call.
static int dp_epoch_close(nfm_opt* o, DpEpoch& de, double* out2, int64_t ns) {
  hipStream_t st = o->ctx->stream;
  NFM_TRY(o->dp_sums.ensure(sizeof(double) * 3));
  double sums[3] = {out2[0], out2[1], (double)ns};
  NFM_HIP_CHECK(hipMemcpyAsync(o->dp_sums.p, sums, sizeof(sums), hipMemcpyHostToDevice, st));
  NFM_TRY(dp_epoch_end(de, o->dp_sums.as<double>()));
  NFM_HIP_CHECK(hipMemcpyAsync(sums, o->dp_sums.p, sizeof(sums), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  out2[0] = sums[0];
  out2[1] = sums[1];
  o->it += (int64_t)(sums[2] + 0.5) - ns;
  return NFM_OK;
}

static int mb_epoch(nfm_opt* o, nfm_model* m, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* out2) {
  nfm_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const ModelView M = m->view();
  const MbCall c = mb_call(o, m, ds, perm, begin, end);
  NFM_TRY(mb_obtain_plan(c));
  // an announced permutation for the next call over the same range: its plan is built beside this epoch.  Every call
  // uses the announcement up, whatever happens to the call after this line.
  const int64_t* announced = o->ahead.take_offer(begin, end);
  if (c.dev_shuffle || o->kind == OPT_PSGD) announced = nullptr;
  DpEpoch de;
  if (o->dp) NFM_TRY(dp_epoch_open(o, m, M, &de));
  DpHooksGuard dp_guard{o};
  // With a plan to build ahead the epoch is only ENQUEUED (its sums go to pinned memory), the build follows on the plan
  // stream, and then the epoch is waited for.  Not with timing enabled (the build's kernels would be timed into the epoch's
  // families); NFM_PLAN_PREFETCH=0: every plan built in line (profiling).
  static const bool prefetch_on = !(getenv("NFM_PLAN_PREFETCH") && atoi(getenv("NFM_PLAN_PREFETCH")) == 0);
  const bool prefetch = (c.dev_shuffle || announced) && !ctx->timing.enabled && prefetch_on;
  if (prefetch) NFM_TRY(o->ahead.ensure_resources());
  double* out2_dst = prefetch ? o->ahead.out2_pinned : out2;
  o->W.rows_ascend = ds->rows_ascend;
  const int rc_epoch = m->cfg.kind == NFM_KIND_FM
                           ? mb_fm_epoch(ctx, o->kind, ds->v, M, o->o, *o->plan, o->W, o->it, out2_dst, (ds->uid << 20) ^ ds->serial, prefetch)
                           : mb_ffm_epoch(ctx, o->kind, ds->v, M, o->o, *o->plan, o->W, o->it, out2_dst, prefetch);
  if (prefetch) {
    // a failed build ahead is reported only after the epoch's own results are in
    const int rc_next = rc_epoch == NFM_OK ? mb_build_ahead(c, announced) : NFM_OK;
    NFM_HIP_CHECK(hipStreamSynchronize(st));
    out2[0] = out2_dst[0];
    out2[1] = out2_dst[1];
    NFM_TRY(rc_next);
  }
  if (c.dev_shuffle) o->shuffle_epoch++;  // (the next call draws the next order even when this epoch failed)
  NFM_TRY(rc_epoch);
  if (o->dp) {
    NFM_TRY(dp_fold_pending(de));  // (SGD: the closing exchange itself brings the arena to true values, scales 1)
    NFM_TRY(dp_epoch_close(o, de, out2, c.ns()));
  }
  dp_guard.ok = true;
  return NFM_OK;
}

static int32_t opt_epoch_range(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin, int64_t end, double* loss_sum,
                               double* viol_sum) {
  nfm_model* m = nullptr;
  NFM_TRY(epoch_call_check(o, ds, perm, begin, end, &m));
  nfm_ctx* ctx = m->ctx;
  if (o->kind == OPT_ADAGRAD) {
    if (o->it == 1 || !o->state_ready) NFM_TRY(adagrad_reset_state(o));
    NFM_TRY(ensure_unit_scale(m));
  } else if (o->kind == OPT_PSGD) {
    NFM_TRY(ensure_unit_scale(m));
  }
  double out2[2] = {0.0, 0.0};
  const int64_t ns = end - begin;
  if (ns > 0) {
    NFM_TRY(o->mode == NFM_MODE_SEQUENTIAL ? seq_epoch(o, m, ds, perm, begin, end, out2) : mb_epoch(o, m, ds, perm, begin, end, out2));
    o->it += o->kind == OPT_PSGD ? ns / o->batch : ns;
    if (o->kind == OPT_SGD && !o->dp) {  // resetScaling, sgd.nim:116-131
      double sc[SC_COUNT];
      NFM_HIP_CHECK(hipMemcpyAsync(sc, m->sc.p, sizeof(sc), hipMemcpyDeviceToHost, ctx->stream));
      NFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (sc[SC_SCALE_P] < 1e-9 || (m->cfg.fit_linear && sc[SC_SCALE_W] < 1e-9)) NFM_TRY(launch_rescale(ctx, m->view()));
    }
  } else if (o->dp) {
    // An empty shard (dp.shard_bounds hands ranks 0 .. W-2 nothing when there are fewer samples than ranks): this rank
    // still issues the collectives its peers wait in -- the agreement on the sync points (it offers none, so the group
    // has none mid-epoch), then the closing exchange with a zero increment -- and leaves with the group's sums and counter.
    NFM_CHECK(o->mode == NFM_MODE_MINIBATCH, NFM_ERR_UNSUPPORTED, "the data-parallel exchange needs NFM_MODE_MINIBATCH");
    DpEpoch de;
    NFM_TRY(dp_epoch_setup(o, m, m->view(), &de));
    NFM_TRY(dp_epoch_begin(de, 0, 0));
    NFM_TRY(dp_epoch_close(o, de, out2, 0));
  }
  if (loss_sum) *loss_sum = out2[0];
  if (viol_sum) *viol_sum = out2[1];
  return NFM_OK;
}

int32_t nfm_opt_predict_all_with_grad(nfm_opt* o, nfm_dataset* ds, double* y_pred, double* dL, double* grad_P, double* grad_w,
                                      double* grad_b, double* loss_sum) {
  NFM_CHECK(o && ds, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(o->kind == OPT_PSGD, NFM_ERR_INVALID, "predictAllWithGrad needs an optimizer made by nfm_mbpsgd_create");
  nfm_model* m = nullptr;
  NFM_TRY(opt_model(o, ds, &m));
  nfm_ctx* ctx = m->ctx;
  NFM_TRY(check_training_data(m, ds));
  NFM_TRY(use_device(ctx));
  NFM_TRY(ensure_unit_scale(m));
  hipStream_t st = ctx->stream;
  const int64_t n = ds->v.n;
  const ModelView M = m->view();
  const size_t bP = pad256(sizeof(double) * std::max<int64_t>(m->nP(), 2)), bw = pad256(sizeof(double) * std::max<int64_t>(m->d, 1));
  DevBuf g, rec2;
  NFM_TRY(g.alloc(bP + bw + 256));
  NFM_HIP_CHECK(hipMemsetAsync(g.p, 0, g.bytes, st));  // features no sample touches keep a zero gradient
  double out2[2] = {0.0, 0.0};
  if (n > 0) {
    MbWork& W = o->Wg;
    NFM_TRY(full_gradient(ctx, ds->v, ds->uid, M, o->o, o->grad_plan, W, g.as<double>(), reinterpret_cast<double*>(g.as<char>() + bP),
                          reinterpret_cast<double*>(g.as<char>() + bP + bw), o->it, out2));
    if (y_pred || dL) {
      NFM_TRY(rec2.alloc(sizeof(double) * 2 * (size_t)n));
      NFM_TRY(mb_fm_records(ctx, W, n, rec2.as<double>(), rec2.as<double>() + n));
      if (y_pred) NFM_HIP_CHECK(hipMemcpyAsync(y_pred, rec2.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
      if (dL) NFM_HIP_CHECK(hipMemcpyAsync(dL, rec2.as<double>() + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (grad_P && m->nP() > 0) {  // device [nb][da][Kp] -> the training layout [nb][da][k]
    DevBuf tmp;
    NFM_TRY(tmp.alloc(sizeof(double) * m->n_ref()));
    NFM_TRY(rows_from_device(m, g.as<double>(), tmp.as<double>(), nullptr));
    NFM_HIP_CHECK(hipMemcpyAsync(grad_P, tmp.p, sizeof(double) * m->n_ref(), hipMemcpyDeviceToHost, st));
    NFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (grad_w) NFM_HIP_CHECK(hipMemcpyAsync(grad_w, g.as<char>() + bP, sizeof(double) * m->d, hipMemcpyDeviceToHost, st));
  if (grad_b) NFM_HIP_CHECK(hipMemcpyAsync(grad_b, g.as<char>() + bP + bw, sizeof(double), hipMemcpyDeviceToHost, st));
  NFM_HIP_CHECK(hipStreamSynchronize(st));
  if (loss_sum) *loss_sum = out2[0];
  return NFM_OK;
}

int32_t nfm_opt_set_shuffle(nfm_opt* o, int64_t seed) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(seed < 0 || o->mode == NFM_MODE_MINIBATCH, NFM_ERR_UNSUPPORTED, "the device-side shuffle needs NFM_MODE_MINIBATCH");
  NFM_CHECK(seed < 0 || o->kind != OPT_CD, NFM_ERR_UNSUPPORTED, "coordinate descent has no sample order to shuffle");
  NFM_CHECK(seed < 0 || o->kind != OPT_PGD, NFM_ERR_UNSUPPORTED, "a full-batch solver has no sample order to shuffle");
  NFM_CHECK(seed < 0 || o->kind != OPT_KATYUSHA, NFM_ERR_UNSUPPORTED, "Katyusha takes its index stream from the host");
  NFM_CHECK(seed < 0 || o->kind != OPT_PSGD_SEQ, NFM_ERR_UNSUPPORTED, "PSGD takes its sample order from the host");
  o->shuffle_seed = seed;
  o->shuffle_epoch = 0;
  o->ahead.invalidate();
  return NFM_OK;
}

int32_t nfm_opt_announce_perm(nfm_opt* o, const int64_t* perm_next, int64_t begin, int64_t end) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(!perm_next || (begin >= 0 && begin < end), NFM_ERR_INVALID, "bad sample range [%lld,%lld)", (long long)begin, (long long)end);
  o->ahead.offer(o->mode == NFM_MODE_MINIBATCH ? perm_next : nullptr, begin, end);
  return NFM_OK;
}

int32_t nfm_opt_get_perm(nfm_opt* o, int64_t* perm, int64_t n) {
  NFM_CHECK(o && (perm || n == 0), NFM_ERR_INVALID, "null argument");
  NFM_CHECK(o->plan && o->plan->has_perm && o->plan->perm.p, NFM_ERR_INVALID, "the last epoch ran in the dataset's own order");
  NFM_CHECK(n == o->plan->end - o->plan->begin, NFM_ERR_INVALID, "the last epoch covered %lld samples, not %lld",
            (long long)(o->plan->end - o->plan->begin), (long long)n);
  NFM_TRY(use_device(o->ctx));
  NFM_HIP_CHECK(hipMemcpyAsync(perm, o->plan->perm.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, o->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(o->ctx->stream));
  return NFM_OK;
}

// ---- a batch plan built for reading back (include/nimfm_hip.h: diagnostic, no optimizer and no model involved) ----
int32_t nfm_dataset_plan_build(nfm_dataset* ds, int32_t n_aug, int32_t order, const int64_t* perm, int64_t seed, int64_t epoch,
                               int64_t begin, int64_t end, int64_t batch, int32_t flags) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  NFM_TRY(refuse_csc(ds, "nfm_dataset_plan_build"));
  NFM_CHECK(order >= NFM_PLAN_ORDER_NONE && order <= NFM_PLAN_ORDER_DEVICE, NFM_ERR_INVALID, "bad order kind");
  NFM_CHECK(order != NFM_PLAN_ORDER_HOST || perm, NFM_ERR_INVALID, "NFM_PLAN_ORDER_HOST without an array");
  NFM_CHECK(n_aug >= 0 && n_aug <= 16, NFM_ERR_INVALID, "bad n_aug");
  NFM_CHECK(flags >= 0 && flags < 16, NFM_ERR_INVALID, "bad flags");
  NFM_CHECK(begin >= 0 && end >= begin, NFM_ERR_INVALID, "bad range");
  nfm_ctx* ctx = ds->ctx;
  NFM_TRY(use_device(ctx));
  if (!ds->diag_plan) ds->diag_plan.reset(new Plan());
  Plan* P = ds->diag_plan.get();
  const PlanKey key{ds->uid, ds->v.nnz, begin, end, batch, (flags & NFM_PLAN_FIRST_SINGLETON) != 0, n_aug, (flags & NFM_PLAN_USE_SINGLES) != 0};
  const bool want_tq = (flags & NFM_PLAN_WANT_TQ) != 0, sort_by_count = (flags & NFM_PLAN_SORT_BY_COUNT) != 0;
  int rc;
  if (order == NFM_PLAN_ORDER_DEVICE) {  // as mb_obtain_plan draws it
    NFM_CHECK(end <= ds->v.n, NFM_ERR_INVALID, "a drawn order covers samples of the dataset");
    DevBuf drawn;
    NFM_TRY(gen_permutation(ctx, ctx->stream, seed, (uint64_t)epoch, begin, end - begin, &drawn));
    const FeistelKey fk = feistel_key(seed, (uint64_t)epoch, begin, end - begin);
    rc = build_plan(ctx, ds, key, want_tq, sort_by_count, P, nullptr, ctx->stream, drawn.as<int64_t>(), &ds->csc, &fk);
    (void)hipStreamSynchronize(ctx->stream);  // `drawn` goes out of scope
  } else {
    const int64_t* ph = order == NFM_PLAN_ORDER_HOST ? perm : nullptr;
    rc = build_plan(ctx, ds, key, want_tq, sort_by_count, P, ph, nullptr, nullptr, ph ? &ds->csc : nullptr);
  }
  if (rc != NFM_OK) ds->diag_plan.reset();
  return rc;
}

int32_t nfm_dataset_plan_get(nfm_dataset* ds, const char* name, void* buf, int64_t capacity, int64_t* count, int32_t* elem_bytes) {
  NFM_CHECK(ds && name, NFM_ERR_INVALID, "null argument");
  NFM_CHECK(ds->diag_plan, NFM_ERR_INVALID, "no plan: nfm_dataset_plan_build comes first");
  const Plan& P = *ds->diag_plan;
  const std::string nm(name);
  const int64_t ns = P.end - P.begin;
  int64_t n = 1;
  int32_t eb = 8;
  const void* host = nullptr;
  const void* dev = nullptr;
  int64_t scalar = 0;
  const std::pair<const char*, int64_t> scalars[] = {
      {"n_batches", P.n_batches}, {"U", P.U}, {"T", P.T}, {"TM", P.TM}, {"max_batch", P.max_batch}, {"max_unique", P.max_unique},
      {"H", P.H}, {"HS", P.HS}, {"max_heavy", P.max_heavy}, {"max_segs", P.max_segs}, {"batch", P.batch},
      {"builder", P.builder}, {"key_bits", P.key_bits}, {"csc_ne", P.csc_ne}, {"csc_by_key", P.csc_by_key ? 1 : 0},
      {"seg_fl", P.seg_fl}, {"seg_nbk", P.seg_nbk}, {"seg_item_bits", P.seg_item_bits}, {"seg_ipt", P.seg_ipt},
      {"seg_s", P.seg_s}, {"seg_xcd", P.seg_xcd}, {"seg_max_cell", P.seg_max_cell},
      {"csc_built", ds->csc.built ? 1 : 0}, {"csc_usable", ds->csc.usable ? 1 : 0}, {"csc_max_col", ds->csc.max_col},
      {"seg_unfit", ds->csc.seg_unfit ? 1 : 0}};
  bool found = false;
  for (const auto& sc : scalars)
    if (nm == sc.first) { scalar = sc.second; host = &scalar; found = true; break; }
  if (!found) {
    const std::pair<const char*, const std::vector<int64_t>*> vecs[] = {
        {"bat_pos", &P.bat_pos}, {"bat_uoff", &P.bat_uoff}, {"bat_toff", &P.bat_toff}, {"bat_hoff", &P.bat_hoff}, {"bat_soff", &P.bat_soff}};
    for (const auto& v : vecs)
      if (nm == v.first) { n = (int64_t)v.second->size(); host = v.second->data(); found = true; break; }
  }
  if (!found) {
    // device arrays: the elements the plan defines (an allocation may be longer: ucol_s and its kin hold max(U, 1))
    struct Arr { const char* name; const DevBuf* b; int32_t eb; int64_t n; };
    const Arr arrs[] = {
        {"perm", &P.perm, 8, ns}, {"ucol", &P.ucol, 4, P.U}, {"uptr", &P.uptr, 8, P.U + 1}, {"ucol_s", &P.ucol_s, 4, P.U},
        {"ubeg_s", &P.ubeg_s, 8, P.U}, {"ucnt_s", &P.ucnt_s, 4, P.U}, {"tpos", &P.tpos, 4, P.TM}, {"tx", &P.tx, 8, P.TM},
        {"tq", &P.tq, 8, P.TM}, {"toff", &P.toff, 8, ns + 1}, {"single", &P.single, 1, P.T}, {"hv_u", &P.hv_u, 8, P.H},
        {"hv_seg0", &P.hv_seg0, 8, P.H > 0 ? P.H + 1 : 0}};
    for (const auto& a : arrs)
      if (nm == a.name) {
        eb = a.eb;
        n = a.b->p ? a.n : 0;  // (an array the build did not make -- an early return, tq not wanted -- has no elements)
        NFM_CHECK((size_t)n * (size_t)eb <= a.b->bytes, NFM_ERR_INVALID, "plan array %s is shorter than the plan says", name);
        dev = a.b->p;
        found = true;
        break;
      }
  }
  NFM_CHECK(found, NFM_ERR_INVALID, "no plan field named %s", name);
  if (count) *count = n;
  if (elem_bytes) *elem_bytes = eb;
  if (!buf) return NFM_OK;
  NFM_CHECK(capacity >= n * eb, NFM_ERR_INVALID, "%s needs %lld bytes, the buffer has %lld", name, (long long)(n * eb), (long long)capacity);
  if (n == 0) return NFM_OK;
  if (host) {
    memcpy(buf, host, (size_t)n * eb);
    return NFM_OK;
  }
  NFM_TRY(use_device(ds->ctx));
  NFM_HIP_CHECK(hipMemcpyAsync(buf, dev, (size_t)n * eb, hipMemcpyDeviceToHost, ds->ctx->stream));
  NFM_HIP_CHECK(hipStreamSynchronize(ds->ctx->stream));
  return NFM_OK;
}

int32_t nfm_dataset_plan_release(nfm_dataset* ds) {
  NFM_CHECK(ds, NFM_ERR_INVALID, "null dataset");
  if (ds->diag_plan) {
    (void)hipSetDevice(ds->ctx->device);
    (void)hipStreamSynchronize(ds->ctx->stream);
    ds->diag_plan.reset();
  }
  return NFM_OK;
}

int32_t nfm_opt_set_dp(nfm_opt* o, nfm_dp* dp, int64_t sync_period, int32_t overlap) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(sync_period >= 0, NFM_ERR_INVALID, "sync_period must be >= 0");
  NFM_CHECK(!dp || dp->ctx == o->ctx, NFM_ERR_INVALID, "optimizer and group belong to different contexts");
  NFM_CHECK(!dp || o->mode == NFM_MODE_MINIBATCH, NFM_ERR_UNSUPPORTED, "the data-parallel exchange needs NFM_MODE_MINIBATCH");
  NFM_CHECK(!dp || o->kind != OPT_PSGD, NFM_ERR_UNSUPPORTED, "MBPSGD has no data-parallel mode");
  NFM_CHECK(!dp || o->kind != OPT_PSGD_SEQ, NFM_ERR_UNSUPPORTED, "PSGD has no data-parallel mode");
  NFM_CHECK(!dp || dp_is_live(dp, dp->uid), NFM_ERR_INVALID, "the group was destroyed");
  o->dp = dp;
  o->dp_uid = dp ? dp->uid : 0;
  o->dp_sync_period = sync_period;
  o->dp_overlap = overlap != 0;
  return NFM_OK;
}

int32_t nfm_opt_set_touch_cap(nfm_opt* o, double cap) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_SGD && o->mode == NFM_MODE_MINIBATCH, NFM_ERR_UNSUPPORTED,
            "the touch cap belongs to SGD in NFM_MODE_MINIBATCH (AdaGrad's state sums every step anyway)");
  NFM_CHECK(cap >= 1.0 && cap == cap, NFM_ERR_INVALID, "touch cap must be >= 1");
  if (o->o.touch_cap != cap) {
    o->o.touch_cap = cap;
    o->W.drop_graph();  // a captured epoch holds the optimizer's parameters by value
  }
  return NFM_OK;
}

int32_t nfm_opt_set_ada_cross(nfm_opt* o, double gamma) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_ADAGRAD && o->mode == NFM_MODE_MINIBATCH, NFM_ERR_UNSUPPORTED,
            "the cross-product weight belongs to AdaGrad in NFM_MODE_MINIBATCH");
  NFM_CHECK(gamma >= 0.0 && gamma == gamma, NFM_ERR_INVALID, "the cross-product weight must be >= 0");
  if (o->o.ada_cross != gamma) {
    o->o.ada_cross = gamma;
    o->W.drop_graph();  // a captured epoch holds the optimizer's parameters by value
  }
  return NFM_OK;
}

int32_t nfm_opt_set_dp_combine(nfm_opt* o, int32_t combine) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(combine == NFM_DP_AUTO || combine == NFM_DP_MEAN || combine == NFM_DP_SUM || combine == NFM_DP_STATE_MEAN || combine == NFM_DP_STATE_RSQRT ||
                combine == NFM_DP_STATE_CROSS,
            NFM_ERR_INVALID, "combine must be NFM_DP_AUTO, NFM_DP_MEAN, NFM_DP_SUM, NFM_DP_STATE_MEAN, NFM_DP_STATE_RSQRT or NFM_DP_STATE_CROSS");
  o->dp_combine = combine;
  return NFM_OK;
}

int32_t nfm_opt_finalize(nfm_opt* o) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  o->ahead.offer(nullptr, 0, 0);  // the end of a fit (or a callback): an announced order refers to an array of the caller's loop
  NFM_TRY(use_device(m->ctx));
  if (o->kind == OPT_PSGD_SEQ) {  // finalize (psgd.nim:58-73), when a fit was begun
    if (o->psgd->fit_ready) NFM_TRY(psgd_seq_finalize(m->ctx, m->view(), o->o, o->psgd.get()));
  } else if (o->kind == OPT_SGD) {
    NFM_TRY(launch_rescale(m->ctx, m->view()));
  } else if (o->kind == OPT_PSGD || o->kind == OPT_CD || o->kind == OPT_PGD || o->kind == OPT_KATYUSHA) {
    // Katyusha: every epoch call leaves finalize's model (katyusha.nim:56-73) in the model handle
    // CD steps the parameters themselves (cd.nim:156-175): nothing to finalise
    // pgd.finalize (optimizer/pgd.nim:45-51) only copies the parameters back
  } else if (o->state_ready) {
    NFM_TRY(launch_adagrad_finalize(m->ctx, m->view(), o->o, o->it));
  }
  NFM_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return NFM_OK;
}

int32_t nfm_opt_device_state(nfm_opt* o, double** gsum_P, double** gnorm_P, int64_t* n_P, double** gsum_w, double** gnorm_w,
                             int64_t* n_w, double** gscalars) {
  NFM_CHECK(o, NFM_ERR_INVALID, "null optimizer");
  NFM_CHECK(o->kind == OPT_ADAGRAD, NFM_ERR_INVALID, "only AdaGrad carries state");
  nfm_model* m = nullptr;
  NFM_TRY(model_of(o, &m));
  if (!o->state_ready) {
    NFM_TRY(use_device(m->ctx));
    NFM_TRY(adagrad_reset_state(o));
  }
  if (gsum_P) *gsum_P = o->G.as<double>();
  if (gnorm_P) *gnorm_P = o->N.as<double>();
  if (n_P) *n_P = m->nP();
  if (gsum_w) *gsum_w = o->Gw.as<double>();
  if (gnorm_w) *gnorm_w = o->Nw.as<double>();
  if (n_w) *n_w = m->d;
  if (gscalars) *gscalars = o->gsc.as<double>();
  return NFM_OK;
}

// ------------------------------------------------------------------ host-side random numbers
// The reference draws P (tensor/tensor.nim:561-580) and shuffles the sample order (optimizer/sgd.nim:297) on the host
// with Nim's global generator.  A Nim host keeps doing exactly that; hosts in other languages (nimfm_amd/host.py,
// nimfm_amd/host/nimfm.hpp) get the same procedures here.  The generator is Nim 1.0's lib/pure/random.nim
// (xoroshiro128+), which is NOT part of the reference tree: restated from memory, unverified.
static inline uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t nim_next(uint64_t* st) {
  const uint64_t s0 = st[0];
  uint64_t s1 = st[1];
  const uint64_t r = s0 + s1;
  s1 ^= s0;
  st[0] = rotl64(s0, 55) ^ s1 ^ (s1 << 14);
  st[1] = rotl64(s1, 36);
  return r;
}
static inline double nim_rand1(uint64_t* st) {  // rand(1.0): 52 random mantissa bits in [1, 2) minus 1
  const uint64_t u = (0x3FFull << 52) | (nim_next(st) >> 12);
  double f;
  memcpy(&f, &u, sizeof(f));
  return f - 1.0;
}

int32_t nfm_rng_randomize(int64_t seed, uint64_t* state) {  // randomize(seed) = initRand(seed)
  NFM_CHECK(state, NFM_ERR_INVALID, "null state");
  state[0] = (uint64_t)seed >> 16;
  state[1] = (uint64_t)seed & 0xffffull;
  (void)nim_next(state);
  return NFM_OK;
}

int32_t nfm_rng_random_normal(uint64_t* state, int64_t n, double loc, double scale, double* out) {
  NFM_CHECK(state && n >= 0 && (out || n == 0), NFM_ERR_INVALID, "null argument");
  // tensor/tensor.nim:561-580: Box-Muller, the two values of one (x, y) draw go to CONSECUTIVE elements of the
  // row-major fill (the pairing runs on across rows and blocks); an odd count leaves the sine half unused
  double x = 0.0, y = 0.0;
  bool has = false;
  const double two_pi = 2 * 3.14159265358979323846;
  for (int64_t t = 0; t < n; ++t) {
    double z;
    if (!has) {
      x = nim_rand1(state);
      y = nim_rand1(state);
      z = sqrt(-2 * log(1.0 - x)) * cos(two_pi * y);
      has = true;
    } else {
      z = sqrt(-2 * log(1.0 - x)) * sin(two_pi * y);
      has = false;
    }
    out[t] = loc + z * scale;
  }
  return NFM_OK;
}

int32_t nfm_rng_shuffle(uint64_t* state, int64_t* x, int64_t n) {
  NFM_CHECK(state && n >= 0 && (x || n == 0), NFM_ERR_INVALID, "null argument");
  // shuffle: for i in countdown(high, 1): swap(x[i], x[rand(i)]); rand(max: int) rejects the top sliver of the
  // 64-bit range and reduces modulo max + 1
  const uint64_t rand_max = ~0ull;
  for (int64_t i = n - 1; i >= 1; --i) {
    uint64_t r;
    do {
      r = nim_next(state);
    } while (r > rand_max - (rand_max % (uint64_t)i));
    const int64_t j = (int64_t)(r % ((uint64_t)i + 1ull));
    const int64_t t = x[i];
    x[i] = x[j];
    x[j] = t;
  }
  return NFM_OK;
}

int32_t nfm_rng_shuffle_forward(uint64_t* state, int64_t* x, int64_t n) {
  NFM_CHECK(state && n >= 0 && (x || n == 0), NFM_ERR_INVALID, "null argument");
  // dataset.nim:388-394: for i in 0..<n: j = rand(n - 1 - i); swap(x[i], x[i + j]); rand(0) returns 0 without a draw
  const uint64_t rand_max = ~0ull;
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t mx = (uint64_t)(n - 1 - i);
    if (mx == 0) continue;
    uint64_t r;
    do {
      r = nim_next(state);
    } while (r > rand_max - (rand_max % mx));
    const int64_t j = (int64_t)(r % (mx + 1ull));
    const int64_t t = x[i];
    x[i] = x[i + j];
    x[i + j] = t;
  }
  return NFM_OK;
}

int32_t nfm_rng_rand_uniform(uint64_t* state, int64_t n, double max, double* out) {  // rand(max: float) = rand(1.0) * max
  NFM_CHECK(state && n >= 0 && (out || n == 0), NFM_ERR_INVALID, "null argument");
  for (int64_t t = 0; t < n; ++t) out[t] = nim_rand1(state) * max;
  return NFM_OK;
}

int32_t nfm_opt_destroy(nfm_opt* o) {
  if (!o) return NFM_OK;
  (void)hipSetDevice(o->ctx->device);
  (void)hipStreamSynchronize(o->ctx->stream);
  o->ahead.release_resources();
  delete o;
  return NFM_OK;
}

}  // extern "C"
