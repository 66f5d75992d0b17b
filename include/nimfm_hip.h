/*
 * include/nimfm_hip.h -- C ABI of libnimfm_hip.so, the MI355X (gfx950) hot path
 * for nimfm factorization machines.
 *
 * The reference (neonnnnn/nimfm, /root/reference) is pure Nim with NO FFI or
 * plugin boundary: `optim.fit(X, y, fm)` and `fm.decisionFunction(X)` are Nim
 * procs resolved at compile time.  This header is therefore the
 * FFI a Nim shim binds with {.importc, cdecl, dynlib.} (nim/nimfm_hip.nim,
 * INTEGRATION.md); each entry point cites the reference proc(s) it replaces.
 * All citations are relative to /root/reference/src/nimfm/.
 *
 * Conventions
 *   - every function returns int32 status: 0 = NFM_OK, < 0 = error; nothing
 *     throws; nfm_last_error() returns a thread-local message.
 *   - plain pointers and sizes only.  Host pointers are caller-owned; the
 *     library copies during the call and keeps nothing host-side.  "*_dev"
 *     pointers are device pointers on the context's GPU.
 *   - one nfm_ctx per GPU per process (one process per GPU); all work of a
 *     context is issued on one HIP stream.  Not thread-safe per context.
 *   - widths follow the reference: Nim int = int64_t, float64 = double.
 *     Parameter layouts at this boundary are the reference's:
 *       FM  P[nOrders][nComponents][nFeatures+nAugments] (model/factorization_machine.nim:31-34)
 *       FFM P[nFields][nFeatures][nComponents]           (model/field_aware_factorization_machine.nim:16-17)
 *       AdaGrad state g_sum/g_norm: P part [nOrders|nFields][nFeatures+nAugments][nComponents],
 *       w part [nFeatures], intercept scalar               (optimizer/adagrad.nim:53-55,155; model/params.nim:5-10)
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with NFM_ERR_HIP.
 */
#ifndef NIMFM_HIP_H
#define NIMFM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFM_OK 0
#define NFM_ERR_INVALID (-1)    /* ValueError in the reference */
#define NFM_ERR_HIP (-2)        /* HIP runtime / no device */
#define NFM_ERR_NOT_FITTED (-3) /* NotFittedError, model/fm_base.nim:13-15 */
#define NFM_ERR_NOMEM (-4)
#define NFM_ERR_UNSUPPORTED (-5)

typedef struct nfm_ctx nfm_ctx;
typedef struct nfm_dataset nfm_dataset;
typedef struct nfm_model nfm_model;
typedef struct nfm_opt nfm_opt;

/* enums mirror the reference's */
enum { NFM_TASK_REGRESSION = 0, NFM_TASK_CLASSIFICATION = 1 };                 /* model/fm_base.nim:6-8 */
enum { NFM_KIND_FM = 0, NFM_KIND_FFM = 1, NFM_KIND_CFM = 2 /* ConvexFactorizationMachine: made by nfm_cfm_create only */ };
enum { NFM_LOWER_EXPLICIT = 0, NFM_LOWER_AUGMENT = 1, NFM_LOWER_NONE = 2 };     /* model/factorization_machine.nim:6-9 */
enum { NFM_LOSS_SQUARED = 0, NFM_LOSS_SQUARED_HINGE = 1, NFM_LOSS_LOGISTIC = 2, NFM_LOSS_HUBER = 3 }; /* loss.nim */
enum { NFM_SCHED_CONSTANT = 0, NFM_SCHED_OPTIMAL = 1, NFM_SCHED_INVSCALING = 2, NFM_SCHED_PEGASOS = 3 }; /* optimizer/sgd.nim:7-11 */
/* NFM_MODE_SEQUENTIAL: one sample at a time in the given order -- the
 *   reference's single-thread semantics (optimizer/sgd.nim:294-308,
 *   optimizer/adagrad.nim:164-184): results equal to the CPU path's.  Run as
 *   a dependency window over the chip (0.9-3.0e6 samples/s; degree-2 FMs,
 *   several orders / degree <= 6, field-aware models; n_components <= 64,
 *   degree-2 FMs <= 128 -- their 128-double rows are read as two blocks of 64;
 *   calls of >= 2048 samples), else one sample in flight (fitLower = augment,
 *   more factors, rows too long for the window's LDS).  With a fitted
 *   intercept the window forms each prediction as intercept + (sum of the
 *   sample's other terms) -- same order, same dependencies, parameters
 *   within ~1e-11 relative of the one-sample-in-flight kernel; the environment
 *   variable NFM_SEQ_WIN_EXACT=1 selects the term-by-term window, BIT-equal to
 *   it (1.2e6 samples/s), NFM_SEQ_WIN_PAR=0 the bitwise-reproducible chain,
 *   NFM_SEQ_WIN=0 the one-sample-in-flight kernel itself.
 * NFM_MODE_MINIBATCH: this library's deterministic data-parallel rule
 *   (DESIGN.md section 4); replaces the reference's racy Hogwild drivers
 *   (optimizer/sgd_multi.nim:40-120, adagrad_multi.nim:39-115); equals the
 *   sequential rule at batch == 1. */
enum { NFM_MODE_SEQUENTIAL = 0, NFM_MODE_MINIBATCH = 1 };
/* sparsity-inducing regularisers (regularizer/l1.nim, l21.nim, squaredl12.nim, squaredl21.nim, omegati.nim).  The first
 * four have a matrix proximal operator and drive MBPSGD; OmegaTI has none (MBPSGD refuses it) and drives PCD only, as
 * L1 and SquaredL12 do (nfm_pcd_create); PBCD takes L1, L21 and SquaredL21 (nfm_pbcd_create) */
enum { NFM_REG_L1 = 0, NFM_REG_L21 = 1, NFM_REG_SQUAREDL12 = 2, NFM_REG_SQUAREDL21 = 3, NFM_REG_OMEGATI = 4, NFM_REG_OMEGACS = 5 };

const char* nfm_last_error(void);
int32_t nfm_version(void);
/* number of visible HIP devices (0 and NFM_OK when none) */
int32_t nfm_device_count(int32_t* n);

/* ---- context: device + stream ---- */
/* hip_stream: a hipStream_t to issue on (e.g. the host framework's current
 * stream), or NULL to let the library create its own. */
int32_t nfm_ctx_create(int32_t device_id, void* hip_stream, nfm_ctx** out);
int32_t nfm_ctx_destroy(nfm_ctx* ctx);
int32_t nfm_ctx_synchronize(nfm_ctx* ctx);
/* per-kernel timing with HIP events on the context's stream (off by default).
 * nfm_ctx_timing_get: accumulated launches / milliseconds of one kernel family
 * ("row_phase", "col_phase", "predict", "sequential", "schedule", ...). */
int32_t nfm_ctx_timing_enable(nfm_ctx* ctx, int32_t on);
int32_t nfm_ctx_timing_reset(nfm_ctx* ctx);
int32_t nfm_ctx_timing_get(nfm_ctx* ctx, const char* family, int64_t* launches, double* total_ms);

/* ---- dataset: CSRDataset / CSRFieldDataset resident in HBM ----
 * replaces tensor/sparse.nim:9-12,19-24 (CSRMatrix, CSRFieldMatrix) +
 * dataset.nim:10-13,182-231 (row iterators incl. dummy features, which the
 * kernels generate on the fly) as the thing `fit`/`decisionFunction` iterate.
 * indices/fields are narrowed to int32 on the device.  y may be NULL for
 * predict-only datasets.  Rows may be stored in any order (dataset.nim:597-612).
 * A column id REPEATED inside a row: decisionFunction / predict / score take
 * it as the reference does (every entry is one more term of the ANOVA
 * recursion, kernels.nim:46-64); TRAINING needs distinct ids per row --
 * nfm_opt_epoch and nfm_opt_predict_all_with_grad return NFM_ERR_UNSUPPORTED
 * naming the first such row.  The reference does not forbid repeats there,
 * but what its step computes for them is an accident of its lazy scaling and
 * scratch layout (the row is rescaled once per ENTRY, optimizer/sgd.nim:134-143;
 * the later entry overwrites the earlier one's derivative dA[j], :176-188, and
 * the row's parameters are then stepped once per entry with it, :217-223);
 * merge repeated entries before training on such a matrix. */
int32_t nfm_dataset_create_csr(nfm_ctx* ctx, int64_t n_samples, int64_t n_features,
                               const int64_t* indptr /*n+1*/, const int64_t* indices /*nnz*/,
                               const double* data /*nnz*/, const int64_t* fields /*nnz or NULL*/,
                               int64_t n_fields, const double* y /*n or NULL*/,
                               nfm_dataset** out);
/* same, adopting arrays that already live on the device (no copy; the caller
 * keeps them alive until nfm_dataset_destroy). */
int32_t nfm_dataset_create_csr_device(nfm_ctx* ctx, int64_t n_samples, int64_t n_features,
                                      int64_t nnz, const int64_t* indptr_dev,
                                      const int32_t* indices_dev, const double* data_dev,
                                      const int32_t* fields_dev, int64_t n_fields,
                                      const double* y_dev, nfm_dataset** out);
/* ---- text ingest, parsed on the GPU ----
 * loadSVMLightFile (dataset.nim:562-632): "target idx:val idx:val ..." per line;
 * loadFFMFile (dataset.nim:696-790): "target field:idx:val ...".  The index
 * base is detected from the file (0-based iff an index 0 occurs, else 1-based,
 * :589/:732-733), nFeatures = max index + 1 - base (nFields likewise); a
 * positive n_features / n_fields smaller than that is NFM_ERR_INVALID (the
 * reference's ValueError, :623-626, :777-785), a larger one wins (:631, :788).
 * A negative index is NFM_ERR_INVALID ("Negative index is included.", :587).
 * Numbers are read as Nim's parseInt / parseFloat read them (correctly rounded
 * binary64).  Targets are stored with the dataset (nfm_dataset_get_targets).
 * nfm_dataset_parse_text: the same from a memory buffer. */
int32_t nfm_dataset_load_svmlight(nfm_ctx* ctx, const char* path, int64_t n_features,
                                  nfm_dataset** out);
int32_t nfm_dataset_load_ffm(nfm_ctx* ctx, const char* path, int64_t n_features, int64_t n_fields,
                             nfm_dataset** out);
int32_t nfm_dataset_parse_text(nfm_ctx* ctx, const char* text, int64_t len, int32_t with_fields,
                               int64_t n_features, int64_t n_fields, nfm_dataset** out);
/* The reference's binary out-of-core format (tensor/sparse_stream.nim:3-33;
 * newStreamCSRDataset, dataset.nim:170-174): "STREAMCSR" | {nRows, nCols, nnz:
 * int64; max, min: float64} | per row nnz: int64 + nnz x {val: float64, id:
 * int64} ("STREAMCSRFIELD": + nFields, elements {field, val, id}).  The whole
 * matrix is made resident in HBM (the reference streams row blocks through a
 * host cache).  y_path: raw float64 labels (loadStreamLabel, dataset.nim:
 * 1007-1014) or NULL.  A STREAMCSC file is NFM_ERR_UNSUPPORTED. */
int32_t nfm_dataset_load_stream(nfm_ctx* ctx, const char* x_path, const char* y_path,
                                nfm_dataset** out);
/* The same files in row blocks, for matrices that do not fit the HBM left over: the reference's out-of-core epoch walks
 * the file through a host-side cache of rows, block by block in file order, without shuffling
 * (readCache, tensor/sparse_stream.nim:232-270; optimizer/sgd_multi.nim:83-97, sgd.nim:297 `if X.nCached ==
 * X.nSamples and self.shuffle`).  nfm_stream_load_rows makes rows [row_begin, row_end) a resident dataset (targets from
 * the label file's rows, zeros without one); the host runs nfm_opt_epoch over block after block -- the optimizer's step
 * counter, scales and state simply continue -- and destroys each block's dataset when it is done with it. */
typedef struct nfm_stream nfm_stream;
int32_t nfm_stream_open(nfm_ctx* ctx, const char* x_path, const char* y_path /*or NULL*/, nfm_stream** out);
int32_t nfm_stream_shape(const nfm_stream* s, int64_t* n_samples, int64_t* n_features, int64_t* nnz, int64_t* n_fields);
int32_t nfm_stream_load_rows(nfm_stream* s, int64_t row_begin, int64_t row_end, nfm_dataset** out);
/* Starts loading rows [row_begin, row_end) in the background (a thread and a HIP stream of the stream object's own: file
 * walk, upload and split run beside the caller's epoch over the current block) and returns at once; the next
 * nfm_stream_load_rows of exactly that range hands the block over (and reports the load's error, if any), any other range
 * drops it.  One block ahead at most.  The reference's readCache (tensor/sparse_stream.nim:232-270) reads the next block
 * only when the epoch loop asks for it (optimizer/sgd_multi.nim:83-97). */
int32_t nfm_stream_prefetch_rows(nfm_stream* s, int64_t row_begin, int64_t row_end);
int32_t nfm_stream_close(nfm_stream* s);
/* convertSVMLightFile (dataset.nim:1017-1097): svmlight text -> STREAMCSR file +
 * raw float64 label file; the text is parsed on the GPU. */
int32_t nfm_convert_svmlight(nfm_ctx* ctx, const char* f_in, const char* f_out_x,
                             const char* f_out_y);
/* ---- datasets made from datasets, without leaving the device ----
 * Every call leaves its inputs untouched and returns a NEW dataset that owns its arrays (destroy it as any other), with
 * the targets of the source rows when the source has them.  All parts of a stack belong to one context and are of one
 * kind (all plain or all field-aware: NFM_ERR_INVALID otherwise).
 * nfm_dataset_select_rows: X[indicesRow] (dataset.nim:319-326, 353-359; tensor/sparse.nim:263-285, 333-357): output row ii
 * is input row rows[ii], its entries in storage order; a row may be taken more than once; n_features and n_fields are
 * kept.  NFM_ERR_INVALID with checkIndicesRow's texts (dataset.nim:307-316): "Invalid slice: nSamples < 1." (m < 1),
 * "max(indicesRow) M >= N.", "min(indicesRow) M < 0.".
 * nfm_dataset_slice_rows: X[begin ..< end] (dataset.nim:328-335, 362-369), the same with rows = begin .. end - 1. */
int32_t nfm_dataset_select_rows(nfm_dataset* ds, const int64_t* rows /*host, m*/, int64_t m, nfm_dataset** out);
int32_t nfm_dataset_slice_rows(nfm_dataset* ds, int64_t begin, int64_t end, nfm_dataset** out);
/* vstack (tensor/sparse.nim:564-581, 613-633): the parts' rows one part after the other; n_fields = the largest of the
 * parts'; targets when EVERY part has them.  NFM_ERR_INVALID "All matrics must have the same shape[1].".
 * hstack (tensor/sparse.nim:671-698, 719-750): row i = the parts' rows i one after the other, column ids offset by the
 * n_features of the parts before, fields by their n_fields; n_features and n_fields are the sums; targets of the FIRST
 * part.  NFM_ERR_INVALID "All matrics must have the same shape[0]."; a summed n_features beyond
 * nfm_dataset_create_csr's bound is NFM_ERR_UNSUPPORTED. */
int32_t nfm_dataset_vstack(nfm_dataset* const* parts, int64_t n_parts, nfm_dataset** out);
int32_t nfm_dataset_hstack(nfm_dataset* const* parts, int64_t n_parts, nfm_dataset** out);
/* normalize (dataset.nim:398-403, tensor/sparse.nim:372-411) into a copy (the reference works in place: a host swaps the
 * handles).  norm: NormKind in the reference's order (tensor/sparse.nim:37-38); axis 1: per row, axis 0: per column.
 * A norm is the reference's fold over the entries in storage order -- x + y^2 then sqrt, x + |y|, max(x, |y|) -- for a
 * column too (its entries in ascending storage position); every entry is divided by its norm when that is != 0.
 * The results are the reference's bits. */
enum { NFM_NORM_L1 = 0, NFM_NORM_L2 = 1, NFM_NORM_LINFTY = 2 };
int32_t nfm_dataset_normalize(nfm_dataset* ds, int32_t axis, int32_t norm, nfm_dataset** out);
/* loadUserItemRatingFile (dataset.nim:840-900), parsed on the GPU: per line the first three runs of digits are user,
 * item (integers) and rating (a float, read from its first digit); any other characters are delimiters and whatever
 * follows the rating is ignored; lines of fewer than 4 characters are skipped.  minUser / minItem start at 1 and
 * maxUser / maxItem at 0 (:863-867); row i = {user - minUser: 1.0, nUsers + item - minItem: 1.0}, n_features = nUsers +
 * nItems, the ratings are the dataset's targets.  NFM_ERR_INVALID where the reference's reading is undefined: a line of
 * exactly 4 characters (its two passes disagree, :853 / :872), a line with fewer than three numbers, ids that do not fit
 * int32, no line at all.  A rating of more than 19 significant digits is NFM_ERR_UNSUPPORTED.
 * nfm_dataset_parse_user_item: the same from a memory buffer. */
int32_t nfm_dataset_load_user_item(nfm_ctx* ctx, const char* path, nfm_dataset** out);
int32_t nfm_dataset_parse_user_item(nfm_ctx* ctx, const char* text, int64_t len, nfm_dataset** out);
/* ---- a dataset on the device -> its text file, formatted on the GPU ----
 * dumpSVMLightFile (dataset.nim:793-805): row i is y_i, then " (j+1):val" per entry in storage order; dumpFFMFile
 * (dataset.nim:825-837): " (field+1):(j+1):val".  "\n" between rows, none after the last; ids 1-based; a float64 as
 * Nim's `$` writes it (the shortest decimal that reads back to the same bits, laid out as Python's repr; "nan", "inf",
 * "-inf").  Rows with repeated or unsorted ids are written as stored.
 * y: host array of n_samples targets, or NULL for the dataset's own; NULL on a dataset without targets is
 * NFM_ERR_INVALID "X.nSamples != len(y)." (:796, :828).  y_int != 0 writes the targets as integers, as the reference
 * does for y: seq[int] (f.write(y[i])); a target that is not integral or not below 2^53 in magnitude is then
 * NFM_ERR_INVALID.  chunk_bytes: the rows are formatted in pieces of at most that much text (a longer row is a piece
 * by itself), the copy to the host and the write of one piece beside the formatting of the next; 0: 128 MiB.
 * nfm_dataset_dump_svmlight on a field-aware dataset and nfm_dataset_dump_ffm on a plain one are NFM_ERR_INVALID, and
 * so is a path that cannot be written. */
int32_t nfm_dataset_dump_svmlight(nfm_dataset* ds, const char* path, const double* y /*host, n, or NULL*/, int32_t y_int,
                                  int64_t chunk_bytes);
int32_t nfm_dataset_dump_ffm(nfm_dataset* ds, const char* path, const double* y /*host, n, or NULL*/, int32_t y_int,
                             int64_t chunk_bytes);
/* the counterpart of nfm_dataset_parse_text: the same bytes into a host buffer of cap bytes (no terminating NUL), the
 * field-aware form for a field-aware dataset.  buf == NULL: the length passes only.  *len: the length of the text;
 * cap < *len is NFM_ERR_INVALID. */
int32_t nfm_dataset_format_text(nfm_dataset* ds, const double* y /*host, n, or NULL*/, int32_t y_int, int64_t chunk_bytes,
                                char* buf /*host, cap, or NULL*/, int64_t cap, int64_t* len);
/* of the calling thread's last nfm_dataset_dump_* / nfm_dataset_format_text: pieces walked, bytes of text, the device ->
 * host copies (HIP events), the file writes / buffer copies and the whole call (host clock), in milliseconds; any
 * pointer may be NULL.  The kernels are timed by nfm_ctx_timing_get's families "dump_len", "dump_scan", "dump_write". */
int32_t nfm_dump_stats(int64_t* pieces, int64_t* bytes, double* copy_ms, double* sink_ms, double* total_ms);
/* n_rows lines of row_len numbers separated by one space, every line ended by "\n": the body of the "P[o]:", "w:" and
 * "lams:" blocks of a model dump (model/factorization_machine.nim:142-165).  buf, cap, len as above. */
int32_t nfm_format_f64(nfm_ctx* ctx, const double* values /*host, n_rows*row_len*/, int64_t n_rows, int64_t row_len,
                       char* buf /*host, cap, or NULL*/, int64_t cap, int64_t* len);
/* the counterpart of nfm_format_f64: the first n_rows lines of text[0, len), row_len numbers each, parsed on the device
 *  -- the "lams:", "P[o]:", "P:" and "w:" blocks `load` reads (model/factorization_machine.nim:168-220,
 * field_aware_factorization_machine.nim:119-158, convex_factorization_machine.nim:111-164).  A token is a maximal run of
 * bytes other than ' ' and '\n'; values[row * row_len + col] is token col of line row, read as a correctly rounded strtod
 * reads it ("-nan" keeps its sign); tokens beyond row_len are read and dropped.  The text goes up in pieces of at most
 * chunk_bytes, each cut at a separator (0: 128 MiB); the upload of one piece and the copy back of another run beside the
 * parse of the one between.  *consumed: the bytes through the n_rows-th '\n', or len when the last line has none.
 * *clean = 0 with NFM_OK: the text is not in that form -- a token that is not a number to its last byte ("5e", "1_0",
 * "1.0\r", a tab) or is longer than 1024 bytes or than a piece, a line of fewer than row_len tokens, fewer than n_rows
 * lines, more than 2^20 tokens left to strtod; values is then unspecified and the caller uses its own parser.  A null
 * argument, a negative shape or length, or n_rows * row_len beyond int64 is NFM_ERR_INVALID.  The kernels are timed by
 * nfm_ctx_timing_get's families "load_index" and "load_parse". */
int32_t nfm_parse_f64(nfm_ctx* ctx, const char* text /*host, len*/, int64_t len, int64_t n_rows, int64_t row_len,
                      int64_t chunk_bytes, double* values /*host, n_rows*row_len*/, int64_t* consumed, int32_t* clean);
/* nfm_dump_stats for the calling thread's last nfm_parse_f64: pieces walked, bytes of text consumed, the uploads (HIP
 * events) and copies back, the staging copies into pinned memory and the whole call (host clock), in milliseconds. */
int32_t nfm_parse_stats(int64_t* pieces, int64_t* bytes, double* copy_ms, double* sink_ms, double* total_ms);
/* ---- column-major datasets (CSCDataset, dataset.nim:18-22) ----
 * A dataset has a layout.  A column-major one owns indptr int64[n_features + 1] (column starts), indices int32[nnz] (sample
 * ids), data f64[nnz] and the optional targets f64[n_samples], and beside them its ROW TWIN: the CSRMatrix toCSRMatrix
 * (tensor/sparse.nim:490-507) makes of it, built on the device when the dataset is made -- one more copy of the matrix in
 * HBM (12 bytes per entry + 8 per sample).  decisionFunction, score, metrics and the column-wise solvers (CD, PCD, PBCD,
 * Hazan, GreedyCD: nfm_cd_*, nfm_hazan_*, nfm_gcd_* and nfm_opt_epoch of such a handle) take a column-major dataset and
 * run on the twin: the reference's column walk adds a sample's terms by ascending column id (kernels.nim:4-44), which is
 * the twin's storage order, so the results are bit-equal to the same call on nfm_dataset_to_csr's result.  A repeated
 * (sample, column) pair predicts and is refused for training, as for any dataset.  nfm_dataset_shape, _get_targets and
 * _set_targets work on both layouts.
 * The row-wise solvers (SGD, AdaGrad, MBPSGD, PSGD, PGD / FISTA / NMAPGD, Katyusha, nfm_opt_predict_all_with_grad and with
 * them a data-parallel group), nfm_dataset_select_rows (tensor/sparse.nim:298: "Accessing row vectors by openarray is not
 * supported for CSCMatrix"), nfm_dataset_dump_* and nfm_dataset_format_text refuse a column-major dataset with
 * NFM_ERR_UNSUPPORTED naming nfm_dataset_to_csr (the reference rejects these at compile time).
 * nfm_dataset_slice_rows (tensor/sparse.nim:300-330: per column the entries with begin <= sample < end, in order, ids
 * rebased), nfm_dataset_hstack (:701-716; "All matrics must have the same shape[0]"), nfm_dataset_vstack (:583-610: per
 * column the parts' columns one after the other, sample ids offset by the earlier parts' n_samples; the result's indptr has
 * n_features + 1 entries where the reference sizes it by shape[0] + 1, :598 -- an index error or an unread tail there) and
 * nfm_dataset_normalize (:414-427: the fold of the row-major call with 1 - axis on the column arrays) take column-major
 * handles and return column-major datasets; a stack that mixes layouts is NFM_ERR_INVALID.
 * nfm_dataset_create_csc: newCSCDataset (dataset.nim:124-129), validated as nfm_dataset_create_csr validates (indptr
 * monotone from 0 to nnz, sample ids in [0, n_samples)); n_samples > 2^31 - 1 is NFM_ERR_UNSUPPORTED.
 * nfm_dataset_to_csc: toCSCDataset (tensor/sparse.nim:510-527) of a row-major dataset: column j lists its entries by
 * ascending sample id, entries of one sample that repeat j in the row's storage order; targets are carried over.  A
 * field-aware dataset and more than 2^31 - 2 entries are NFM_ERR_UNSUPPORTED.  nfm_dataset_to_csr: toCSRDataset
 * (:490-507), the mirror image, of a column-major dataset.  A dataset that already has the layout asked for is copied.
 * nfm_dataset_get_csc: the column arrays in the reference's widths (CSCMatrix, tensor/sparse.nim:14-17); any pointer may
 * be NULL; NFM_ERR_INVALID for a row-major dataset. */
enum { NFM_LAYOUT_CSR = 0, NFM_LAYOUT_CSC = 1 };
int32_t nfm_dataset_create_csc(nfm_ctx* ctx, int64_t n_samples, int64_t n_features,
                               const int64_t* indptr /*d+1*/, const int64_t* indices /*nnz*/,
                               const double* data /*nnz*/, const double* y /*n or NULL*/, nfm_dataset** out);
/* same, from column arrays that already live on the device.  Unlike nfm_dataset_create_csr_device the arrays are COPIED
 * (the dataset owns its columns and its twin; the caller may free them on return); indptr is checked, the sample ids are
 * trusted to be in range. */
int32_t nfm_dataset_create_csc_device(nfm_ctx* ctx, int64_t n_samples, int64_t n_features, int64_t nnz,
                                      const int64_t* indptr_dev, const int32_t* indices_dev, const double* data_dev,
                                      const double* y_dev, nfm_dataset** out);
int32_t nfm_dataset_to_csc(nfm_dataset* ds, nfm_dataset** out);
int32_t nfm_dataset_to_csr(nfm_dataset* ds, nfm_dataset** out);
int32_t nfm_dataset_layout(const nfm_dataset* ds, int32_t* layout);
int32_t nfm_dataset_get_csc(nfm_dataset* ds, int64_t* indptr /*d+1*/, int64_t* indices /*nnz*/, double* data /*nnz*/);
/* nfm_dataset_load_user_item / _parse_user_item with the line rule as a switch: short_lines != 0 skips lines of fewer than
 * 5 characters, as loadUserItemRatingFile for a CSCDataset does in all three of its passes (dataset.nim:923, 955, 975) -- a
 * line of exactly 4 characters is then skipped, not refused.  The result is row-major; the column-major loader is this
 * with short_lines = 1 followed by nfm_dataset_to_csc (dataset.nim:903-992 makes exactly that matrix). */
int32_t nfm_dataset_load_user_item_lines(nfm_ctx* ctx, const char* path, int32_t short_lines, nfm_dataset** out);
int32_t nfm_dataset_parse_user_item_lines(nfm_ctx* ctx, const char* text, int64_t len, int32_t short_lines, nfm_dataset** out);
/* ---- the binary stream files, written and transposed on the device ----
 * The format is tensor/sparse_stream.nim:3-33: magic | {nRows, nCols, nnz[, nFields]: int64; max, min: float64} | per record
 * an int64 count and count x {val: float64, id: int64} (field-aware: {field: int64, val, id}).  The records are packed into
 * those bytes by a kernel, in pieces of at most chunk_bytes (0: 128 MiB) cut at record boundaries -- a longer record is a
 * piece by itself -- and the copy to the host and the write of one piece run beside the packing of the next.
 * nfm_dataset_dump_stream: a row-major plain dataset -> "STREAMCSR", a field-aware one -> "STREAMCSRFIELD", a column-major
 * one -> "STREAMCSC" (one record per column, ids = sample ids).  nRows / nCols are n_samples / n_features in all three, as
 * transposeFile writes them and newStreamCSCMatrix reads them.  max / min are the reference's fold over the values in
 * storage order from -Inf / +Inf (dataset.nim:1021-1022, 1052-1053): a NaN never replaces a bound and of +0.0 / -0.0 the
 * first stays.  The targets are not part of the file.  nfm_dump_stats reports the call (kernel: family "stream_pack").
 * nfm_dataset_format_stream: the same bytes into a host buffer; buf, cap, len as nfm_dataset_format_text.
 * nfm_dataset_load_stream_csc: newStreamCSCDataset (dataset.nim:176-179) + loadStreamLabel (:1007-1014): a "STREAMCSC" file
 * becomes a column-major dataset (with its row twin), resident as a whole.  The file is validated as
 * nfm_dataset_load_stream validates: header sizes against the file length, a column that overruns the file, summed counts
 * against nnz, ids outside [0, nRows), the label count against nRows (NFM_ERR_INVALID).  A "STREAMCSR..." file is
 * NFM_ERR_UNSUPPORTED naming nfm_dataset_load_stream.
 * nfm_transpose_file: transposeFile (dataset.nim:1100-1199) in either direction: "STREAMCSR" -> "STREAMCSC" and back.  The
 * 40 header bytes are copied as they are (:1122-1124): max / min are not recomputed, nRows / nCols not swapped.  Output
 * record j lists the entries with id j by ascending input record, entries of one input record that repeat j in storage
 * order: the reference's result when its cache holds every entry (with a smaller cache its loop writes wrong files or
 * raises an index error; the hosts accept cacheSize and ignore it).  A file whose first output record would be empty,
 * nnz = 0 included, is NFM_ERR_INVALID: the reference does not terminate on it (:1150, 1190-1196).  A "...FIELD" file is
 * NFM_ERR_UNSUPPORTED (the reference compares 9 magic bytes and would read it as a plain file); there is no
 * transposeFieldFile.  More than 2^31 - 2 entries or 2^31 - 1 records: NFM_ERR_UNSUPPORTED, as nfm_dataset_to_csc.
 * nfm_convert_ffm: convertFFMFile (dataset.nim:1202-1299): libffm text -> "STREAMCSRFIELD" file + raw float64 labels.  ids
 * are shifted by minIndex (initial 1), nCols = maxIndex - minIndex + 1; the fields are NOT shifted (:1287 against :1294)
 * while nFields = maxField - minField + 1 (initial 1 / 0) -- so a file with 1-based fields carries a field equal to nFields,
 * which nfm_dataset_load_stream refuses; 0-based fields round-trip.  NFM_ERR_INVALID "Negative field index is included."
 * before "Negative index is included." (:1249-1252). */
int32_t nfm_dataset_dump_stream(nfm_dataset* ds, const char* path, int64_t chunk_bytes);
int32_t nfm_dataset_format_stream(nfm_dataset* ds, int64_t chunk_bytes, char* buf /*host, cap, or NULL*/, int64_t cap, int64_t* len);
int32_t nfm_dataset_load_stream_csc(nfm_ctx* ctx, const char* x_path, const char* y_path /*or NULL*/, nfm_dataset** out);
int32_t nfm_transpose_file(nfm_ctx* ctx, const char* f_in, const char* f_out, int64_t chunk_bytes);
int32_t nfm_convert_ffm(nfm_ctx* ctx, const char* f_in, const char* f_out_x, const char* f_out_y);
/* nSamples / nFeatures / nnz / nFields (dataset.nim:44-51, tensor/sparse.nim:26-40) */
int32_t nfm_dataset_shape(const nfm_dataset* ds, int64_t* n_samples, int64_t* n_features,
                          int64_t* nnz, int64_t* n_fields);
/* 1 where every row stores its column ids in strictly ascending order, else 0.  Established once, when the dataset is
 * made, by the pass that looks for repeated ids; the mini-batch kernels choose by it how a batch's linear weights are staged. */
int32_t nfm_dataset_rows_ascend(const nfm_dataset* ds, int32_t* ascend);
/* bytes of text, upload and parse time of the loader that made this dataset */
int32_t nfm_dataset_ingest_stats(const nfm_dataset* ds, int64_t* bytes, double* upload_ms,
                                 double* parse_ms);
/* read-back in the reference's widths (CSRMatrix data/indices/indptr, fields:
 * tensor/sparse.nim:9-12,19-24); any pointer may be NULL */
int32_t nfm_dataset_get_targets(nfm_dataset* ds, double* y /*n*/);
int32_t nfm_dataset_get_csr(nfm_dataset* ds, int64_t* indptr /*n+1*/, int64_t* indices /*nnz*/,
                            double* data /*nnz*/, int64_t* fields /*nnz*/);
/* model/fm_base.nim:29-36 checkTarget is applied by the optimizer according to
 * the model's task; this replaces the targets (host array, n). */
int32_t nfm_dataset_set_targets(nfm_dataset* ds, const double* y);
int32_t nfm_dataset_destroy(nfm_dataset* ds);

/* ---- model: FactorizationMachine / FieldAwareFactorizationMachine ---- */
typedef struct nfm_model_cfg {
  int32_t kind;          /* NFM_KIND_* */
  int32_t task;          /* NFM_TASK_* */
  int32_t degree;        /* FM only; FFM is degree 2 */
  int32_t n_components;  /* k -- no cap for FactorizationMachines: above 128 the factors of an order
                          * are kept as blocks of at most 128 on the device (an ANOVA kernel is a sum over
                          * the factors, kernels.nim:46-64), the layouts at this boundary stay the
                          * reference's; decisionFunction, SGD and AdaGrad in both modes take such models
                          * (MBPSGD does not: its matrix prox needs a feature's factors in one row).
                          * Field-aware models: k <= 128 outside NFM_MODE_SEQUENTIAL. */
  int32_t fit_lower;     /* NFM_LOWER_* (FM only) */
  int32_t fit_intercept;
  int32_t fit_linear;
  int32_t reserved;
  int64_t n_features;    /* d (without augments) */
  int64_t n_fields;      /* FFM only */
} nfm_model_cfg;

/* newFactorizationMachine (model/factorization_machine.nim:43-78) /
 * newFieldAwareFactorizationMachine (model/field_aware_factorization_machine.nim:24-46):
 * NFM_ERR_INVALID if degree < 1 or n_components < 1 (:65-69). */
int32_t nfm_model_create(nfm_ctx* ctx, const nfm_model_cfg* cfg, nfm_model** out);
/* nOrders / nAugments (model/factorization_machine.nim:81-97); for FFM
 * n_blocks = nFields and n_aug = 0. */
int32_t nfm_model_shape(const nfm_model* m, int32_t* n_blocks, int32_t* n_aug);
/* fm.init's result / a loaded model (model/factorization_machine.nim:125-139,
 * 183-220): marks the model initialised.  lams may be NULL (= ones, :78). */
int32_t nfm_model_set_params(nfm_model* m, const double* P, const double* w, double intercept,
                             const double* lams);
/* finalised parameters in the reference layout (what fm.P / fm.w /
 * fm.intercept hold after fit; optimizer/sgd.nim:327-328).  For AdaGrad call
 * nfm_opt_finalize first. */
int32_t nfm_model_get_params(nfm_model* m, double* P, double* w, double* intercept);
/* decisionFunction (model/factorization_machine.nim:100-122 -> kernels.nim:14-19,
 * 46-64; FFM: model/field_aware_factorization_machine.nim:52-76).
 * NFM_ERR_NOT_FITTED when not initialised, NFM_ERR_INVALID on nFeatures /
 * nFields mismatch (:114-115, FFM :60-64).  out: n doubles. */
int32_t nfm_decision_function(nfm_model* m, nfm_dataset* ds, double* out);
int32_t nfm_decision_function_device(nfm_model* m, nfm_dataset* ds, double* out_dev);
/* score (model/fm_base.nim:39-48): rmse for regression, accuracy of the signs for
 * classification, of decisionFunction(ds) against the dataset's targets -- computed
 * on the device, only the scalar comes back. */
int32_t nfm_score(nfm_model* m, nfm_dataset* ds, double* out);
/* metrics.nim:5-13 (rmse), :39-47 (accuracy of signs), :76-103 (rocauc, pos = 1) of
 * decisionFunction(ds) against the dataset's targets; any pointer may be NULL. */
int32_t nfm_metrics(nfm_model* m, nfm_dataset* ds, double* rmse, double* accuracy, double* rocauc);
/* ---- every pair of two row sets, and the K best per row ----
 * cross[i][j] is decisionFunction (model/factorization_machine.nim:100-122, kernels.nim:59-64) of the row "row i of dsU
 * followed by row j of dsV with its column ids moved up by dsU's nFeatures" -- row i * nV + j of hstack(U[repeat], V[tile]),
 * tensor/sparse.nim:671-698 -- without that dataset being made; the dummy feature of fitLower = augment is appended once
 * (:112).  dsU.nFeatures + dsV.nFeatures must be the model's nFeatures: NFM_ERR_INVALID "Invalid nFeatures." (:114-115).
 * A FactorizationMachine of degree 2 on resident CSR / CSC datasets of one context; NFM_ERR_UNSUPPORTED, naming the way
 * that remains (the pairs and nfm_decision_function), for any other degree, field-aware and convex models, field-aware
 * datasets and dsU / dsV of different contexts.  The bits of cross[i][j] depend on the two rows and the model alone.
 * out: nU * nV doubles on the host (copied out in blocks of users; NFM_ERR_UNSUPPORTED when so many scores do not fit the
 * device: use nfm_cross_topk or row slices of dsU). */
int32_t nfm_cross_decision_function(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, double* out);
/* the same (model/factorization_machine.nim:100-122, kernels.nim:59-64, tensor/sparse.nim:671-698) into device memory:
 * out_dev holds nU * nV doubles; complete on return. */
int32_t nfm_cross_decision_function_device(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, double* out_dev);
/* Per row i of dsU the K pairs (j, cross[i][j]) -- the scores of nfm_cross_decision_function bit for bit
 * (model/factorization_machine.nim:100-122, kernels.nim:59-64, tensor/sparse.nim:671-698), never written to memory -- by
 * descending score, then ascending j; a NaN score ranks below every number, NaN against NaN by j.
 * 1 <= K <= min(nV, 256), else NFM_ERR_INVALID.  chunk_items: the items one workgroup ranks for its users, rounded up to
 * whole tiles of 64; 0 = the library's choice; the result does not depend on it.  ids, scores: host, [nU][K]. */
int32_t nfm_cross_topk(nfm_model* m, nfm_dataset* dsU, nfm_dataset* dsV, int64_t K, int64_t chunk_items, int64_t* ids, double* scores);
/* ||P||^2 and ||w||^2 for optimizer/utils.nim:56-59 `regularization` (verbose). */
int32_t nfm_model_sqnorms(nfm_model* m, double* P_sq, double* w_sq);
/* device views for the data-parallel exchange: pointers to
 * the device-layout parameter buffers and their lengths in doubles. scalars
 * holds {scale_P, scale_w, intercept, 5 unused}. (Device layout: FM [nOrders][d+nAug][Kp], FFM [d][nFields][Kp]
 * with Kp >= k zero-padded -- opaque to an element-wise exchange.) The three buffers are pieces of
 * ONE allocation in the order [P | w | scalars] (gaps are zero padding), so a
 * single collective over [P_dev, scalars_dev + n_scalars) reconciles a replica. */
int32_t nfm_model_device_buffers(nfm_model* m, double** P_dev, int64_t* n_P, double** w_dev,
                                 int64_t* n_w, double** scalars_dev, int64_t* n_scalars);
int32_t nfm_model_destroy(nfm_model* m);

/* ---- optimizers ---- */
typedef struct nfm_sgd_cfg { /* newSGD, optimizer/sgd.nim:23-52 */
  double eta0, alpha0, alpha, beta, power, loss_param /* Huber threshold */;
  int32_t loss, scheduling, mode, reserved;
  int64_t batch; /* NFM_MODE_MINIBATCH only */
} nfm_sgd_cfg;

typedef struct nfm_adagrad_cfg { /* newAdaGrad, optimizer/adagrad.nim:20-44 */
  double eta0, alpha0, alpha, beta, eps, loss_param;
  int32_t loss, mode, track_viol /* 1 = keep the reference's sum|dP| (adagrad.nim:99) */, reserved;
  int64_t batch;
} nfm_adagrad_cfg;

/* newMBPSGD (optimizer/minibatch_psgd.nim:24-65): the reference's own mini-batch rule --
 * the gradient of `batch` samples averaged (updateGradient, :67-84), one step on ALL parameters
 * (Params.step, model/params.nim:90-98), then the regulariser's prox per order with
 * gamma * eta_P / (1 + eta_P * beta) (:112-120).  FactorizationMachine only.  SquaredL12 / SquaredL21 need
 * degree 2 (their initSGD raises, squaredl12.nim:103-105); reg_transpose: SquaredL12 column-wise (1, the
 * reference default) or row-wise (0); SquaredL21 only 0 (its default).
 * nfm_opt_epoch on such an optimizer runs (end - begin) / batch mini-batches over perm[begin..end) -- the
 * stream of sample indices the reference's inner loops consume (indices[ii], wrap-arounds included), so
 * end may exceed nSamples when perm is given and (end - begin) must be a multiple of batch; `it` advances
 * once per mini-batch (:121); viol_sum is 0 (the solver has none). */
typedef struct nfm_mbpsgd_cfg {
  double eta0, alpha0, alpha, beta, gamma, power, loss_param;
  int32_t loss, scheduling, reg /* NFM_REG_* */, reg_transpose;
  int64_t batch; /* miniBatchSize >= 1 */
} nfm_mbpsgd_cfg;

int32_t nfm_sgd_create(nfm_model* m, const nfm_sgd_cfg* cfg, nfm_opt** out);
int32_t nfm_adagrad_create(nfm_model* m, const nfm_adagrad_cfg* cfg, nfm_opt** out);
int32_t nfm_mbpsgd_create(nfm_model* m, const nfm_mbpsgd_cfg* cfg, nfm_opt** out);
/* newPSGD (optimizer/psgd.nim:23-55) with newL1() or newL21(): SGD in the reference's sample order, one sample at a time,
 * plus a sparsity regulariser whose effect on the rows a sample does not touch is caught up lazily (l1.nim:80-136,
 * l21.nim:64-113).  The config is nfm_mbpsgd_cfg -- newPSGD takes newMBPSGD's hyper-parameters; batch and reg_transpose are
 * ignored.  reg: NFM_REG_L1 or NFM_REG_L21.  NFM_ERR_UNSUPPORTED: NFM_REG_SQUAREDL12 / NFM_REG_SQUAREDL21 (their step touches
 * every parameter per sample: nfm_mbpsgd_create has them -- newPSGD()'s own default, newSquaredL12(), is among these),
 * NFM_REG_OMEGATI / NFM_REG_OMEGACS (no SGD hooks), a field-aware or convex model, n_components > 128, degree > 6.
 * nfm_psgd_begin_fit is reg.initSGD and psgd.nim:97-98: every fit starts from fresh caches (scalings = 1, thresholds = 0,
 * scalings_w = 1); only `it` persists between fits (nfm_opt_set_it / nfm_opt_get_it, psgd.nim:106-107).  Rows must hold
 * distinct column ids (NFM_ERR_UNSUPPORTED); they need not be sorted.
 * Then nfm_opt_epoch(o, ds, perm, begin, end, &loss_sum, &viol_sum) runs psgd.nim:122-184 over perm[begin .. end) (perm NULL:
 * the dataset's order), 0 <= begin <= end <= nSamples: loss_sum = sum of loss(y_i, yPred_i) taken before each step, viol_sum
 * = 0 (the solver has none); `it` advances by end - begin.  A call without begin_fit on that dataset is NFM_ERR_INVALID.
 * Consecutive calls continue each other: an epoch is any sequence of its sub-ranges.
 * nfm_psgd_finalize is finalize (psgd.nim:58-73): the catch-up of w, then reg.lazyUpdateFinal -- before every callback and
 * at the end of fit; nfm_opt_finalize does the same on such a handle.  After it nfm_model_get_params returns the reference's
 * fm.P / fm.w / fm.intercept.
 * One departure: L1's cache reset (l1.nim:113-126, scaling < 1e-8) applies lazyUpdateFinal's formula, as finalize and L21's
 * own reset do; the reference's lines are not a catch-up and overflow on the steps that follow. */
int32_t nfm_psgd_create(nfm_model* m, const nfm_mbpsgd_cfg* cfg, nfm_opt** out);
int32_t nfm_psgd_begin_fit(nfm_opt* o, nfm_dataset* ds);
int32_t nfm_psgd_finalize(nfm_opt* o);
/* predictAllWithGrad (optimizer/pgd.nim:70-103), the full-batch half of the proximal solvers, on an optimizer made
 * by nfm_mbpsgd_create (its loss is used; its state and `it` are untouched): y_pred[n] = the model's output on every
 * sample, dL[n] = dloss(y_i, y_pred_i), and the gradient of the MEAN loss -- grad_P in the training layout
 * [nOrders][d + nAugments][k] (the reference's grads.P), grad_w[d] (zeros unless fitLinear), *grad_b (0 unless
 * fitIntercept), *loss_sum = sum_i loss(y_i, y_pred_i).  Any output pointer may be NULL. */
int32_t nfm_opt_predict_all_with_grad(nfm_opt* o, nfm_dataset* ds, double* y_pred, double* dL,
                                      double* grad_P, double* grad_w, double* grad_b, double* loss_sum);
/* newCD (optimizer/cd.nim:12-25): coordinate descent for a FactorizationMachine (NFM_ERR_UNSUPPORTED for a field-aware model;
 * the reference has no CD for it).  alpha0 / alpha / beta as newCD takes them (the fit scales them by nSamples, cd.nim:117-127);
 * loss: NFM_LOSS_*, loss_param: Huber's threshold.  The features run as a level schedule: features that
 * share no sample step in parallel, every sample sees its features' steps in the reference's ascending order, so the
 * parameters are the reference's -- bit for bit for the rows' features; the intercept and the dummy features of
 * fitLower = augment sum over all samples with a fixed tree.
 * nfm_cd_begin_fit (cd.nim:128-153): the schedule of the dataset (built once per dataset and kept), colNormSq and yPred
 * from the model's current parameters and the dataset's current targets (sign()-ed for classification).  Then every
 * nfm_opt_epoch(o, ds, NULL, 0, nSamples, &loss_sum, &viol_sum) is ONE iteration (cd.nim:156-175): loss_sum = sum_i
 * loss(y_i, yPred_i) after it, viol_sum = the reference's viol.  A non-NULL perm, another range, or a call without a
 * begin_fit on that dataset (and its current targets) is NFM_ERR_INVALID; shuffling, data-parallel groups, the touch cap
 * and the cross-product weight are NFM_ERR_UNSUPPORTED; nfm_opt_finalize does nothing.  Rows must hold distinct column
 * ids (NFM_ERR_UNSUPPORTED); they need not be sorted.
 * nfm_cd_schedule: the depth (number of levels) and the widest level of the P sweep's schedule on ds, the augments'
 * levels (one each) included. */
int32_t nfm_cd_create(nfm_model* m, double alpha0, double alpha, double beta, int32_t loss, double loss_param, nfm_opt** out);
int32_t nfm_cd_begin_fit(nfm_opt* o, nfm_dataset* ds);
int32_t nfm_cd_schedule(nfm_opt* o, nfm_dataset* ds, int64_t* n_levels, int64_t* widest_level);
/* newPCD (optimizer/pcd.nim:17-35): proximal coordinate descent, CD's loop with a proximal step per feature
 * (pcd.nim:38-104).  gamma: the sparsity strength (scaled by nSamples as the others, pcd.nim:137); reg: NFM_REG_L1
 * (l1.nim:25-27), NFM_REG_SQUAREDL12 (squaredl12.nim:127-131,166-188; reg_transpose != 0 is newSquaredL12()'s default,
 * the column-wise penalty) or NFM_REG_OMEGATI (omegati.nim:40-66).  L21 and SquaredL21 are NFM_ERR_UNSUPPORTED
 * (nimfm_sparsefm.nim:124-146 refuses them for PCD) and so is NFM_REG_OMEGACS (it has no CD hooks); SquaredL12 with degree != 2 is NFM_ERR_INVALID (initCD,
 * squaredl12.nim:91-93).  Every feature with invStepSize < 1e-12 is skipped, at every degree (pcd.nim:57,100).
 * The handle is a CD handle: nfm_cd_begin_fit, nfm_opt_epoch and nfm_cd_schedule work on it with CD's rules and errors.
 * L1 and row-wise SquaredL12 keep CD's level schedule; column-wise SquaredL12 and OmegaTI read a running value over
 * every earlier feature, so their P sweep runs as a run schedule: runs of consecutive features
 * that share no sample, the proximal chain walked in ascending j.  nfm_cd_schedule then reports the runs (the augments'
 * runs of one included) and the widest run. */
int32_t nfm_pcd_create(nfm_model* m, double alpha0, double alpha, double beta, double gamma, int32_t loss, double loss_param,
                       int32_t reg, int32_t reg_transpose, nfm_opt** out);
/* newPBCD (optimizer/pbcd.nim:20-46): proximal block coordinate descent at maxSearch = 0, the reference's default
 * (pbcd.nim:112-209,212-329).  A feature's whole row P[j, 0..k) steps at once: one walk of the schedule per order and
 * iteration.  alpha0 and alpha are scaled by nSamples (pbcd.nim:226-227), beta and gamma are NOT (:138,147,154).  reg:
 * NFM_REG_L1 (l1.nim:31-33), NFM_REG_L21 (l21.nim:25-29) -- both on CD's level schedule -- or NFM_REG_SQUAREDL21
 * (squaredl21.nim:32-43,90-101, transpose = false; degree 2 only, initBCD :68-73: another degree is NFM_ERR_INVALID), whose
 * prox reads the running sum of every row's norm and runs the run schedule, or NFM_REG_OMEGACS
 * (omegacs.nim:31-85; any degree), whose prox reads the running ANOVA polynomials of every row's norm: the run schedule
 * too, with its cache and dcache resident on the device for the whole fit.  NFM_REG_SQUAREDL12
 * and NFM_REG_OMEGATI are NFM_ERR_UNSUPPORTED (nimfm_sparsefm.nim:118), and so is max_search != 0 (the line search,
 * pbcd.nim:80-109).  The intercept and the w sweep are CD's (fit_linear.nim:5-37).
 * The handle is a CD handle: nfm_cd_begin_fit, nfm_opt_epoch and nfm_cd_schedule work on it with CD's rules and errors;
 * nfm_cd_schedule reports runs for SquaredL21 and OmegaCS and levels otherwise.  loss_sum is the fixed-tree sum after the iteration
 * where the reference keeps a running total (pbcd.nim:185-187). */
int32_t nfm_pbcd_create(nfm_model* m, double alpha0, double alpha, double beta, double gamma, int32_t loss, double loss_param,
                        int32_t reg, int32_t max_search, nfm_opt** out);

/* newPGD, newFISTA, newNMAPGD (optimizer/pgd.nim:19-42, fista.nim:20-43, nmapgd.nim:20-46): the full-batch proximal
 * gradient solvers of a FactorizationMachine.  Every parameter set of the fit loops (params, old_params, grads; FISTA's
 * z_params; NMAPGD's y, z, old_x, old_y, old_y_grads, x_grads) stays on the device; per line-search trial one record of a
 * few doubles comes back and the library takes the branch on the host.
 * The hyper-parameters are scalars, as nfm_pcd_create and nfm_pbcd_create take theirs.  reg: NFM_REG_L1, NFM_REG_L21, NFM_REG_SQUAREDL12 (reg_transpose != 0: column-wise, the
 * reference default) or NFM_REG_SQUAREDL21 (reg_transpose == 0 only).  SquaredL12 / SquaredL21 with degree != 2 are
 * NFM_ERR_INVALID (initSGD, squaredl12.nim:103-105); NFM_REG_OMEGATI and NFM_REG_OMEGACS (no matrix prox), a field-aware model, and
 * n_components > 128 with another regulariser than L1 are NFM_ERR_UNSUPPORTED; rho outside (0, 1) is NFM_ERR_INVALID (the
 * unbounded search, max_search <= 0, then ends after at most log(1e-12) / log(rho) + 1 trials, pgd.nim:119,138).
 * algo == NFM_PGD_ALGO_NMAPGD: alpha0 is ignored and alpha used in its place (nmapgd.nim:44 stores alpha0: alpha); eta is
 * its non-monotonicity, not a step size.  The column-coupled operators use the deterministic threshold iteration of MBPSGD
 * in place of the reference's randomised pivoting (same result to rounding).
 * nfm_pgd_begin_fit (pgd.nim:164-183, fista.nim:67-98, nmapgd.initCaches :49-76 and the initial c :208-215): buffers, the
 * one-batch plan, the caches.  warm_start = the model's warmStart: FISTA keeps t, NMAPGD keeps t, c, q and its caches.
 * Then every nfm_opt_epoch(o, ds, NULL, 0, nSamples, &loss_sum, &viol_sum) is ONE iteration, line search included
 * (pgd.nim:186-203, fista.nim:99-127, nmapgd.nim:221-247): loss_sum = lossVal * nSamples, viol_sum = computeViol (the SQUARED
 * distance the reference compares with tol).  After it the model handle holds `params` (what pgd.finalize copies out).
 * A non-NULL perm, another range, or a call without begin_fit on that dataset is NFM_ERR_INVALID; shuffling, data-parallel
 * groups and the touch cap are NFM_ERR_UNSUPPORTED; rows must hold distinct column ids (NFM_ERR_UNSUPPORTED).
 * nfm_pgd_last_iter: out[NFM_PGD_IT_COUNT] of the last iteration -- lossVal, regVal, viol; the step size each line search
 * ended with and its number of trials (NMAPGD: the Z search, then the V search, 0 trials when it did not run); the branch
 * (NFM_PGD_BRANCH_*); t, and NMAPGD's c and q after the iteration; the step size each line search STARTED from (1 for PGD
 * and FISTA, getStepSize's Barzilai-Borwein ratio for NMAPGD, nmapgd.nim:89-99), so that the final step size is that start
 * multiplied by rho once per shrink, exactly. */
enum { NFM_PGD_ALGO_PGD = 0, NFM_PGD_ALGO_FISTA = 1, NFM_PGD_ALGO_NMAPGD = 2 };
enum { NFM_PGD_BRANCH_NONE = 0, NFM_PGD_BRANCH_ACCEPT = 1, NFM_PGD_BRANCH_RESTART = 2, NFM_PGD_BRANCH_Z = 3, NFM_PGD_BRANCH_V = 4 };
enum { NFM_PGD_IT_LOSS = 0, NFM_PGD_IT_REG = 1, NFM_PGD_IT_VIOL = 2, NFM_PGD_IT_ETA = 3, NFM_PGD_IT_ETA_V = 4, NFM_PGD_IT_TRIALS = 5,
       NFM_PGD_IT_TRIALS_V = 6, NFM_PGD_IT_BRANCH = 7, NFM_PGD_IT_T = 8, NFM_PGD_IT_C = 9, NFM_PGD_IT_Q = 10, NFM_PGD_IT_START = 11,
       NFM_PGD_IT_START_V = 12, NFM_PGD_IT_COUNT = 13 };
int32_t nfm_pgd_create(nfm_model* m, int32_t algo, double alpha0, double alpha, double beta, double gamma, double rho, double sigma,
                       double eta, int32_t loss, double loss_param, int32_t reg, int32_t reg_transpose, int64_t max_search, nfm_opt** out);
int32_t nfm_pgd_begin_fit(nfm_opt* o, nfm_dataset* ds, int32_t warm_start);
int32_t nfm_pgd_last_iter(nfm_opt* o, double* out);
/* newKatyusha (optimizer/katyusha.nim:24-53): the variance-reduced accelerated proximal solver of a FactorizationMachine.
 * params, z, y, tilde, next_tilde, grads_ave and the mini-batch gradients stay on the device; per
 * outer iteration only {loss_sum, viol_sum} come back.  The hyper-parameters are scalars, as nfm_pgd_create takes its own.
 * batch >= 1 is miniBatchSize as the host resolved it (katyusha.nim:203-206); tau1 and tau2 are passed as the user gave
 * them: tau2 < 0 is 1 / (2 batch), tau1 < 0 is tau2 (:208-213).  reg as for nfm_pgd_create, with the same refusals.
 * NFM_ERR_INVALID: eta <= 0; beta <= 0, alpha <= 0 with fit_linear, alpha0 <= 0 with fit_intercept (the scale of next_tilde,
 * (1 - theta) / (1 - theta^m), :150-152, is 0 / 0 there: the reference returns NaN parameters); batch outside [1, 2^31-1] or
 * an epoch's index stream of more than 2^31-1 positions; tau1, tau2 that make finalize's divisor zero.
 * nfm_katyusha_begin_fit (:182-219): the sets, y, z, tilde <- the model's parameters, maxIterInner =
 * (nSamples - 1) / batch + 1, the first predictAllWithGrad.  Nothing is carried between fits.
 * Then every nfm_opt_epoch(o, ds, perm, begin, end, &loss_sum, &viol_sum) is ONE outer iteration (:229-262) over the index
 * stream perm[begin .. end): end - begin must be batch * maxIterInner (NFM_ERR_INVALID otherwise), end may exceed nSamples
 * as for MBPSGD, perm == NULL is the identity stream with wrap-around.  loss_sum = sum_i loss(y_i, yPred_i) at the
 * snapshot the iteration STARTED from (:241-244), viol_sum = computeViol(next_tilde, tilde) (:235).  After it the model
 * handle holds what finalize (:56-73, with the arguments as fit passes them, :238, :269) gives the user.  The full gradient
 * at the new snapshot (:261-262) is taken at the start of the NEXT call.  nfm_opt_finalize does nothing.
 * A call without begin_fit on that dataset and its current targets is NFM_ERR_INVALID; shuffling on the device,
 * data-parallel groups and the touch cap are NFM_ERR_UNSUPPORTED; rows must hold distinct column ids (NFM_ERR_UNSUPPORTED). */
int32_t nfm_katyusha_create(nfm_model* m, double eta, double alpha0, double alpha, double beta, double gamma, double tau1, double tau2,
                            int32_t loss, double loss_param, int32_t reg, int32_t reg_transpose, int64_t batch, nfm_opt** out);
int32_t nfm_katyusha_begin_fit(nfm_opt* o, nfm_dataset* ds);
/* tilde_params, the snapshot the verbose line's regVal is taken on (katyusha.nim:250-252): P[nOrders][d + nAugments][k] in the
 * training layout, w[d], *intercept; any of them may be NULL. */
int32_t nfm_katyusha_snapshot(nfm_opt* o, double* P, double* w, double* intercept);

/* ---- ConvexFactorizationMachine and Hazan's algorithm ----
 * newConvexFactorizationMachine (model/convex_factorization_machine.nim:25-46): a model handle of kind NFM_KIND_CFM with
 * room for max_components basis vectors; NFM_ERR_INVALID "maxComponents < 1." (:37-38).  The handle carries P
 * [n_components][n_features] row-major, lams [n_components], w [n_features] and the intercept; n_components starts at 0
 * (init, :49-60) and grows to max_components.  ignore_diag != 0: the ANOVA kernel (kernels.nim:22-43), else the polynomial
 * kernel (:67-79), both of degree 2.
 * nfm_cfm_set_params: a loaded or warm-started model (:111-164); 0 <= n_components <= max_components; P and lams may be NULL
 * when n_components == 0.  Marks the model initialised.
 * nfm_cfm_get_params: *n_components, then P [n_components][n_features], lams [n_components], w, *intercept; size P and lams
 * for max_components.  Any pointer may be NULL.
 * nfm_decision_function(_device), nfm_score and nfm_metrics take such a handle (:63-84): linear + intercept, then
 * lams[s] * K[s] component by component, every row summed in storage order; zero components are legal.
 * nfm_model_set_params / nfm_model_get_params / nfm_model_sqnorms / nfm_model_device_buffers and every other optimizer
 * refuse it (NFM_ERR_UNSUPPORTED). */
int32_t nfm_cfm_create(nfm_ctx* ctx, int32_t task, int32_t max_components, int32_t fit_intercept, int32_t fit_linear,
                       int32_t ignore_diag, int64_t n_features, nfm_model** out);
int32_t nfm_cfm_set_params(nfm_model* m, int32_t n_components, const double* P, const double* lams, const double* w,
                           double intercept);
int32_t nfm_cfm_get_params(nfm_model* m, int32_t* n_components, double* P, double* lams, double* w, double* intercept);
/* newHazan (optimizer/hazan.nim:22-46) for a NFM_KIND_CFM handle (anything else: NFM_ERR_UNSUPPORTED); squared loss only.
 * maxIter, tol, nTol, verbose and self.it stay with the host's loop (:136-138,198-225).
 * nfm_hazan_begin_fit (:63-134): the column twin of the dataset (built once per dataset), colNormSq, yPredLinear, K and
 * yPredQuad of the components the handle holds, the residual; *loss_old = ||residual||^2 / nSamples (:133).  Targets are
 * sign()-ed for classification.  Rows must hold distinct column ids (NFM_ERR_UNSUPPORTED).
 * nfm_hazan_iter (:140-202): ONE outer iteration.  it = self.it (the step size 2 / (it + 2) when optimal == 0, :56);
 * start: the power method's start vector, n_features doubles as drawn (2 * rand(1.0) - 1 each, tensor/tensor.nim:920-921;
 * the library normalises it, :922).  The power method (:924-933) and the conjugate gradient (:990-1007 as :186 calls it)
 * run in chunks of iterations, each chunk one captured single-stream graph whose launches do nothing once the stop flag
 * in device memory is set; the host reads the flag between chunks.  Everything else of the iteration is a fixed sequence
 * of launches.  record[NFM_HAZAN_REC_COUNT]: lossNew (:202), the trace norm (:207), the slot s (:145-147), the step size
 * (:165), the power iterations run, the CG iterations run (completed updates of x), the last eval, n_components after.
 * The one deliberate deviation: the reference's cg never leaves on its iteration cap (tensor.nim:992 does not increment
 * `it`); here the loop ends after 1000 iterations, and when curv is 0 or not finite.
 * A call without begin_fit on that dataset and its current targets is NFM_ERR_INVALID.  nfm_opt_epoch on such an optimizer
 * is NFM_ERR_INVALID. */
enum { NFM_HAZAN_REC_LOSS = 0, NFM_HAZAN_REC_TRACE = 1, NFM_HAZAN_REC_SLOT = 2, NFM_HAZAN_REC_STEP = 3, NFM_HAZAN_REC_POWER_ITERS = 4,
       NFM_HAZAN_REC_CG_ITERS = 5, NFM_HAZAN_REC_EVAL = 6, NFM_HAZAN_REC_N_COMPONENTS = 7, NFM_HAZAN_REC_COUNT = 8 };
int32_t nfm_hazan_create(nfm_model* m, double eta, int64_t max_iter_power, double tol_power, int32_t optimal, nfm_opt** out);
int32_t nfm_hazan_begin_fit(nfm_opt* o, nfm_dataset* ds, double* loss_old);
int32_t nfm_hazan_iter(nfm_opt* o, nfm_dataset* ds, int64_t it, const double* start, double* record);
/* ---- GreedyCD for the convex factorization machine ----
 * newGreedyCD (optimizer/greedy_cd.nim:25-30) at refitFully = false, for a NFM_KIND_CFM handle (anything else:
 * NFM_ERR_UNSUPPORTED).  alpha0, alpha, beta are the caller's; the solver steps scale them by nSamples (:424-426), the outer
 * objective does not (:455-457).  loss: NFM_LOSS_*, loss_param: Huber's threshold.  maxIter, maxIterInner, nRefitting, tol and
 * verbose stay with the host's loops, and so does every stopping decision.  yPred, dL, K [max_components][nSamples], P, lams,
 * w, colNormSq and the power method's vectors stay on the device; the power method is Hazan's, with dL as the weight vector
 * (:338-345), and runs in the same captured chunks.
 * nfm_gcd_create: refit_fully != 0 is accepted here and refused by nfm_gcd_begin_fit with NFM_ERR_UNSUPPORTED (:388-390 needs
 * ADMM, Newton-CG and LAPACK's dsyev: it stays with the reference).
 * nfm_gcd_begin_fit (:419-457): the column twin of the dataset and its levels, colNormSq, K of the components the handle holds,
 * yPred = linear + intercept + sum lams[s] K[s]; *loss_old = sum loss / nSamples, *reg_old = 0.5 alpha0 b^2 + 0.5 alpha
 * norm(w, 2)^2 + beta ||lams||_1.  Targets are sign()-ed for classification.
 * nfm_gcd_outer_begin (:464-469, :332-336): fitInterceptCD, fitLinearCD (the coordinate-descent kernels, over the twin), then
 * fitZ's head; record holds N_COMPONENTS (the count of NON-ZERO lams), OBJECTIVE ((sum loss + beta n ||lams||_1) / n) and
 * N_STORED.
 * nfm_gcd_inner (:347-397): ONE inner iteration of fitZ.  start: the power method's start vector, n_features doubles as drawn
 * (2 * rand(1.0) - 1 each), given exactly when the last record's N_COMPONENTS < max_components and NULL otherwise
 * (NFM_ERR_INVALID if not so): with it, dL, the power method, the slot (the first s with lams[s] == 0, else appended), K[s],
 * fitLams (:76-94) and yPred += lams[s] K[s] when the new lams[s] != 0.  A component thresholded to zero stays stored.
 * refit != 0: refitDiag (:97-109) over every stored component; a zero lams[s] is skipped on the device.  record: ADDED (1 when
 * a base with a non-zero lams was added), SLOT (-1 without a start vector), LAM (the slot's new lams), POWER_ITERS (the
 * reference's count), EVAL, N_COMPONENTS, OBJECTIVE (:394-397, computed in every call), N_STORED (the handle's n_components).
 * nfm_gcd_outer_end (:474-476, :493-497): *loss and *reg as at begin_fit; recompute != 0 rebuilds yPred = linear + intercept +
 * sum lams[s] K[s], components in ascending s.
 * The calls of one outer iteration come in this order; one out of order, or without begin_fit on that dataset and its current
 * targets, is NFM_ERR_INVALID.  nfm_opt_epoch on such an optimizer is NFM_ERR_INVALID. */
enum { NFM_GCD_REC_ADDED = 0, NFM_GCD_REC_SLOT = 1, NFM_GCD_REC_LAM = 2, NFM_GCD_REC_POWER_ITERS = 3, NFM_GCD_REC_EVAL = 4,
       NFM_GCD_REC_N_COMPONENTS = 5, NFM_GCD_REC_OBJECTIVE = 6, NFM_GCD_REC_N_STORED = 7, NFM_GCD_REC_COUNT = 8 };
int32_t nfm_gcd_create(nfm_model* m, double alpha0, double alpha, double beta, int32_t loss, double loss_param, int64_t max_iter_power,
                       double tol_power, int32_t refit_fully, nfm_opt** out);
int32_t nfm_gcd_begin_fit(nfm_opt* o, nfm_dataset* ds, double* loss_old, double* reg_old);
int32_t nfm_gcd_outer_begin(nfm_opt* o, nfm_dataset* ds, double* record);
int32_t nfm_gcd_inner(nfm_opt* o, nfm_dataset* ds, const double* start, int32_t refit, double* record);
int32_t nfm_gcd_outer_end(nfm_opt* o, nfm_dataset* ds, int32_t recompute, double* loss, double* reg);
/* the optimizer's `it` (optimizer/sgd.nim:18,55-56; adagrad.nim:14,50): starts
 * at 1, +1 per sample; set to 1 to mimic a non-warm-start fit. */
int32_t nfm_opt_set_it(nfm_opt* o, int64_t it);
int32_t nfm_opt_get_it(nfm_opt* o, int64_t* it);
/* AdaGrad g_sum / g_norm (optimizer/adagrad.nim:15-16), reference layout. */
int32_t nfm_opt_get_state(nfm_opt* o, double* gsum_P, double* gnorm_P, double* gsum_w,
                          double* gnorm_w, double* gsum_b, double* gnorm_b);
int32_t nfm_opt_set_state(nfm_opt* o, const double* gsum_P, const double* gnorm_P,
                          const double* gsum_w, const double* gnorm_w, double gsum_b,
                          double gnorm_b);
/* The body of one epoch of fit (optimizer/sgd.nim:298-308, adagrad.nim:169-184;
 * FFM: sgd_ffm.nim:77-87, adagrad_ffm.nim:35-48) over samples
 * perm[begin..end) (perm NULL = identity; perm is the host-side shuffle,
 * sgd.nim:297).  Sub-ranges serve nCalls callbacks (sgd.nim:303-307).  Returns
 * the running sums the reference prints/tests: sum of loss(y_i, yhat_i) and
 * `viol`.  Classification targets are sign()-ed (fm_base.nim:32-34).
 * A range of more than 2^31 - 1 entries is walked as consecutive pieces
 * (whole mini-batches): the results are the one call's (not with a
 * data-parallel group attached; a device-drawn order shuffles inside a piece). */
int32_t nfm_opt_epoch(nfm_opt* o, nfm_dataset* ds, const int64_t* perm, int64_t begin,
                      int64_t end, double* loss_sum, double* viol_sum);
/* shuffle = true on the device (NFM_MODE_MINIBATCH): with seed >= 0 every nfm_opt_epoch call WITHOUT an explicit
 * permutation runs over a fresh random order of the samples [begin, end), drawn on the device from (seed, number of
 * such calls so far) -- the reference shuffles `indices` on the host once per epoch (optimizer/sgd.nim:297, Nim's global
 * generator, not reproduced: RNG parity is unpinned either way) -- and the batch plan of the NEXT such call is built on a
 * second stream while the current epoch runs.  seed < 0 switches it off (the default: perm == NULL is the dataset's own
 * order).  nfm_opt_get_perm: the n = end - begin sample ids of the most recent epoch call that ran in a permuted order
 * (device-drawn or passed in), so that any run can be replayed sample for sample. */
int32_t nfm_opt_set_shuffle(nfm_opt* o, int64_t seed);
/* A host that shuffles itself (the Nim host: shuffle(indices), optimizer/sgd.nim:297) can tell the library the
 * permutation of the NEXT epoch before it runs the current one: nfm_opt_announce_perm(o, perm_next, begin, end), then
 * nfm_opt_epoch(o, ds, perm_current, begin, end, ...).  The plan for perm_next is built on a second stream beside the
 * current epoch and used when the next nfm_opt_epoch call passes the SAME array (same pointer, same range); the array
 * must stay alive and unchanged until that call returns (so the host alternates between two index arrays).  An
 * announcement that is not followed up costs only the wasted build.  NFM_MODE_MINIBATCH; ignored otherwise. */
int32_t nfm_opt_announce_perm(nfm_opt* o, const int64_t* perm_next, int64_t begin, int64_t end);
int32_t nfm_opt_get_perm(nfm_opt* o, int64_t* perm /*n*/, int64_t n);
/* ---- reading a batch plan back (diagnostic, read-only: no optimizer and no model is involved) ----
 * Every mini-batch epoch runs on a batch plan: the batch boundaries and, per batch, the feature-major view of its rows
 * that the column phase walks.  nfm_dataset_plan_build builds one by the function the epoch
 * calls, for the samples [begin, end) of a row-major dataset, and keeps it with the dataset (replacing an earlier one;
 * nfm_dataset_plan_release or nfm_dataset_destroy lets it go).
 *   order: NFM_PLAN_ORDER_NONE the dataset's own order; NFM_PLAN_ORDER_HOST `perm`, indexed as the epoch indexes it
 *     (position p of the range is sample perm[begin + p]; the range may pass the end of the data, the ids may repeat);
 *     NFM_PLAN_ORDER_DEVICE the order nfm_opt_set_shuffle's epochs draw on the device from (seed, epoch).
 *   With an order the dataset's column-major twin is offered to the build exactly as the epoch offers it.
 *   flags: NFM_PLAN_* below, or-ed.
 * nfm_dataset_plan_get hands a field back by name: *count elements of *elem_bytes bytes each, copied to buf when buf is
 * not NULL (capacity: its size in bytes; NFM_ERR_INVALID when too small).  Names:
 *   int64 scalars  n_batches U T TM max_batch max_unique H HS max_heavy max_segs batch, and who built the plan:
 *                  builder (NFM_PLAN_BY_*), key_bits (the sort's key width this build was instantiated for),
 *                  csc_ne csc_by_key (twin: entries per lane 4 / 8 / 16, positions computed from the order's key),
 *                  seg_fl seg_nbk seg_max_cell (bucketing, also when it was tried and gave up: bucket width 2^fl, buckets,
 *                  largest cell), seg_item_bits seg_ipt seg_s seg_xcd (bucketing: item width, items per thread, samples
 *                  per chunk, one XCD per batch); of the dataset: csc_built csc_usable csc_max_col seg_unfit
 *   int64 vectors  bat_pos bat_uoff bat_toff bat_hoff bat_soff (n_batches + 1 each; bat_hoff / bat_soff empty when the
 *                  build returned early)
 *   device arrays  perm int64[end - begin]; ucol int32[U]; uptr int64[U + 1]; ucol_s int32[U]; ubeg_s int64[U];
 *                  ucnt_s int32[U]; tpos int32[TM]; tx double[TM]; tq int64[TM]; toff int64[end - begin + 1];
 *                  single uint8[T]; hv_u int64[H]; hv_seg0 int64[H + 1] (none without heavy features).  An array the
 *                  build did not make (no order, tq not wanted, an empty range ...) has 0 elements. */
enum { NFM_PLAN_ORDER_NONE = 0, NFM_PLAN_ORDER_HOST = 1, NFM_PLAN_ORDER_DEVICE = 2 };
enum { NFM_PLAN_FIRST_SINGLETON = 1, NFM_PLAN_WANT_TQ = 2, NFM_PLAN_USE_SINGLES = 4, NFM_PLAN_SORT_BY_COUNT = 8 };
enum { NFM_PLAN_BY_SORT = 0, NFM_PLAN_BY_TWIN = 1, NFM_PLAN_BY_SEG = 2 };
int32_t nfm_dataset_plan_build(nfm_dataset* ds, int32_t n_aug, int32_t order, const int64_t* perm, int64_t seed, int64_t epoch,
                               int64_t begin, int64_t end, int64_t batch, int32_t flags);
int32_t nfm_dataset_plan_get(nfm_dataset* ds, const char* name, void* buf, int64_t capacity, int64_t* count, int32_t* elem_bytes);
int32_t nfm_dataset_plan_release(nfm_dataset* ds);
/* finalize (optimizer/sgd.nim:99-113; adagrad.nim:65-84): leaves the model's
 * parameters as the reference's fm.P/w/intercept after fit. Idempotent. */
int32_t nfm_opt_finalize(nfm_opt* o);
/* device views of the AdaGrad state for the data-parallel exchange; pieces of ONE
 * allocation in the order [gsum_P | gnorm_P | gsum_w | gnorm_w | gscalars]
 * (gaps are zero padding): [gsum_P, gscalars + 2) is one collective. */
int32_t nfm_opt_device_state(nfm_opt* o, double** gsum_P, double** gnorm_P, int64_t* n_P,
                             double** gsum_w, double** gnorm_w, int64_t* n_w,
                             double** gscalars /* {gsum_b, gnorm_b} */);
int32_t nfm_opt_destroy(nfm_opt* o);

/* ---- data-parallel groups: sample shards, replicated parameters, periodic exchange ----
 * Replaces the reference's Hogwild drivers (optimizer/sgd_multi.nim:40-120, adagrad_multi.nim:39-115,
 * sgd_ffm_multi.nim, adagrad_ffm_multi.nim: T threads, contiguous sample slices `nSamples div nThreads`,
 * ONE shared unsynchronised model) across GPUs: rank r trains on its own contiguous slice, resident in its GPU's
 * HBM (the host hands each rank its slice as that rank's nfm_dataset), the model is replicated, and nfm_opt_epoch
 * reconciles the replicas every `sync_period` mini-batches and exactly at the end of the call:
 *   SGD      replicas averaged;
 *   AdaGrad  the replicas' g_sum / g_norm increments since the last exchange summed (the state ONE process would hold
 *            after all shards' samples, optimizer/adagrad.nim:113-134).
 * With overlap != 0 a mid-epoch exchange is delayed by one period: the collective runs on the group's own stream beside
 * the next period's mini-batches and its result is folded in at the next sync point (a fixed point: results are
 * reproducible).  All ranks of a group call nfm_opt_epoch together, with equal step counters at the call's start; the
 * call returns the loss / viol sums over ALL ranks (sgd_multi.nim:98-101) and advances the step counter by the samples
 * of all ranks (the reference's threads share one counter, sgd_multi.nim:37).  After the call all replicas hold the
 * same bits.  NFM_MODE_MINIBATCH, SGD and AdaGrad (FM and FFM).
 *
 * nfm_dp_create: one PROCESS per GPU; the collective is ncclAllReduce(ncclDouble) of RCCL over xGMI on the single
 * parameter / state arena.  Rank 0 obtains an id with nfm_dp_unique_id and the host distributes its
 * NFM_DP_ID_BYTES bytes (file, environment, MPI, torch.distributed ...); nfm_dp_create is collective.
 * nfm_dp_create_local: `world` ranks inside ONE process, one nfm_ctx (and one host thread) each -- several GPUs with
 * peer access, or one GPU shared by all ranks; the collective is a rendezvous of the ranks' host threads and a
 * rank-ordered device-side sum.  out receives `world` handles. */
typedef struct nfm_dp nfm_dp;
#define NFM_DP_ID_BYTES 128
int32_t nfm_dp_unique_id(void* id /*[NFM_DP_ID_BYTES]*/);
int32_t nfm_dp_create(nfm_ctx* ctx, const void* id /*[NFM_DP_ID_BYTES]*/, int32_t rank, int32_t world, nfm_dp** out);
int32_t nfm_dp_create_local(nfm_ctx* const* ctxs /*[world]*/, int32_t world, nfm_dp** out /*[world]*/);
/* rank / world of the group, collectives issued and bytes contributed so far (any pointer may be NULL) */
int32_t nfm_dp_info(const nfm_dp* dp, int32_t* rank, int32_t* world, int64_t* n_collectives, int64_t* bytes);
int32_t nfm_dp_destroy(nfm_dp* dp);
/* attach (dp != NULL) or detach (dp == NULL) a group; sync_period: mini-batches between exchanges, 0 = only the exact
 * exchange at the end of every nfm_opt_epoch call */
int32_t nfm_opt_set_dp(nfm_opt* o, nfm_dp* dp, int64_t sync_period, int32_t overlap);  /* detach before nfm_dp_destroy */
/* How SGD combines the ranks' increments at an exchange (AdaGrad always adds its state increments up):
 * NFM_DP_MEAN (default) -- the replicas' mean: local SGD, as stable as one rank, but the model moves as far as ONE rank's
 * steps take it; NFM_DP_SUM -- every rank's steps land in the model, as every Hogwild thread's steps land in the
 * reference's shared one (optimizer/sgd_multi.nim:83-101): the progress of all ranks' steps, at the price of a step size
 * that is effectively multiplied by the number of ranks wherever their features overlap (keep sync_period small).
 * DESIGN.md section 6 has the measurements. */
/* AdaGrad: the state increments are SUMMED by default (with an exchange after every mini-batch that is synchronous
 * data-parallel AdaGrad -- the state ONE process would hold).  With long periods every rank fits its own shard between
 * exchanges and the summed state over-shoots by up to the number of ranks (measured: 4 ranks x 16 mini-batches between
 * exchanges left the held-out RMSE at 2.9 where one rank reaches 1.04, tools/dp_convergence.py); NFM_DP_STATE_MEAN averages
 * the ranks' state increments instead -- the replicas' mean, as stable as one rank at any period.
 * NFM_DP_AUTO (the default of every optimizer, so a host that only calls nfm_opt_set_dp gets it): SGD -- the mean;
 * AdaGrad -- the sum when sync_period == 1, NFM_DP_STATE_CROSS otherwise (sync_period 0 included; rounds 3-4: the averaged state).
 * NFM_DP_STATE_RSQRT: the ranks' increments weighted by 1 / sqrt(world) -- between the sum (weight 1) and the mean (1 / world). */
/* NFM_DP_STATE_CROSS (AdaGrad, round 5): g_sum increments summed; g_norm += sum_r dN_r + gamma ((sum_r dG_r)^2 - sum_r dG_r^2),
 * gamma = 0.1, never less than before -- the cross products of the ranks' increments inflate the norm where the ranks pushed the
 * same way from the same stale point (there the plain sum over-shoots) and vanish where they saw different things.  One
 * all-reduce of the same size (a rank sends dN_r - gamma dG_r^2 for dN_r).  Keeps one rank's progress per epoch at 2 / 4 / 8
 * ranks for every period, a whole epoch included (profiles/r05g_dp_convergence.txt); NFM_DP_AUTO picks it for AdaGrad beyond
 * one mini-batch per exchange. */
enum { NFM_DP_AUTO = -1, NFM_DP_MEAN = 0, NFM_DP_SUM = 1, NFM_DP_STATE_MEAN = 2, NFM_DP_STATE_RSQRT = 3, NFM_DP_STATE_CROSS = 4 };
int32_t nfm_opt_set_dp_combine(nfm_opt* o, int32_t combine);

/* SGD, NFM_MODE_MINIBATCH: how a mini-batch combines the per-sample steps (optimizer/sgd.nim:205-243) of the `c` samples
 * that touch one coordinate.  The reference's Hogwild threads (optimizer/sgd_multi.nim:83-101, maxThreads of them) each
 * apply their step at full strength to a shared model that is at most maxThreads steps stale.  Here: up to `cap` of a
 * batch's steps on a coordinate are SUMMED; a coordinate touched c > cap times receives cap / c of the sum (and cap / c
 * of the batch's decay exponent).  cap = 1 (the default) is the per-coordinate MEAN: always stable, but one epoch then
 * makes about 1 / c_bar of the sequential order's progress, c_bar = mean touch count per touched coordinate.  cap =
 * the reference's thread count gives its staleness; 16 matched one sequential epoch's held-out loss per epoch on the
 * bench workloads and stayed stable where the plain sum (cap = infinity) diverges on dense coordinates and the
 * intercept.  Larger mini-batches want the cap to follow: with cap about twice the batch's mean touch
 * count per coordinate (batch * nnz-per-row / n_features) the epochs to a held-out loss stay those of the sequential order
 * (measured up to 32 at batch 262144 of the headline shape and 64 at 524288, profiles/r05h_touch_cap_sweep.txt); a cap
 * below that rate turns the tail of the batch into the mean.  Deterministic for every value. */
int32_t nfm_opt_set_touch_cap(nfm_opt* o, double cap);
/* AdaGrad, NFM_MODE_MINIBATCH (round 5): what a mini-batch adds to a coordinate's g_norm (optimizer/adagrad.nim:122-124 adds
 * g^2 per sample).  All samples of a batch take their gradients from the batch-start parameters; summing their squares alone
 * does not see whether they agree, and a coordinate touched by many samples of a batch that push the same way is then stepped
 * as far as if the samples had been independent observations -- field-aware AdaGrad at batch 32768 needed 13 / 28 / more than
 * 40 epochs for the held-out loss of 1 / 3 / 10 epochs in the reference's order.  With gamma > 0 the norm grows by
 *   sum_i g_i^2 + gamma * max((sum_i g_i)^2 - sum_i g_i^2, 0)
 * -- the cross products of the batch's gradients (what squaring the batch gradient does in large-batch AdaGrad, and what
 * NFM_DP_STATE_CROSS does for the ranks of a group): 2 / 4 / 11 epochs at batch 32768, as at batch 2048.
 * A coordinate touched once is not affected, so batch == 1 stays the reference's step.  gamma = 0 (default): off.
 * Deterministic for every value. */
int32_t nfm_opt_set_ada_cross(nfm_opt* o, double gamma);

/* ---- host-side random numbers (no device work) ----
 * FactorizationMachine.init draws P with randomNormal (model/factorization_machine.nim:125-139,
 * tensor/tensor.nim:561-580: Box-Muller over rand(1.0); z = sqrt(-2 ln(1-x)) cos(2 pi y) and the sine twin go
 * to CONSECUTIVE elements of the row-major fill [nOrders][nComponents][nFeatures+nAugments] (FFM:
 * [nFields][nFeatures][nComponents]), an odd count leaves the twin unused) after randomize(randomState);
 * fit shuffles the sample order with the same global generator (optimizer/sgd.nim:297).  A Nim host keeps
 * calling Nim's own procs; these entry points give hosts in other languages the same procedures.  state is the
 * generator's two 64-bit words.  The generator (Nim 1.0 lib/pure/random.nim, xoroshiro128+) is outside the
 * reference tree and restated from memory: the PROCEDURE (pairing, fill order, shuffle loop) follows the
 * reference, the bit stream is unverified. */
int32_t nfm_rng_randomize(int64_t seed, uint64_t* state /*[2]*/);
int32_t nfm_rng_random_normal(uint64_t* state, int64_t n, double loc, double scale, double* out /*n*/);
int32_t nfm_rng_shuffle(uint64_t* state, int64_t* x, int64_t n);
/* The permutation draw of shuffle(X, y) (dataset.nim:388-394): for i ascending, j = rand(n - 1 - i), swap(x[i], x[i + j])
 * -- NOT Nim's shuffle, which counts down (nfm_rng_shuffle).  Same generator, same caveat: the procedure follows the
 * reference, the bit stream is unverified. */
int32_t nfm_rng_shuffle_forward(uint64_t* state, int64_t* x, int64_t n);
/* n draws of rand(max) (a uniform float in [0, max], Nim's rand(max: float)) in sequence: the power method's start vector is
 * 2 * rand(1.0) - 1 per feature from the global generator (tensor/tensor.nim:920-921), nFeatures draws per outer iteration
 * of Hazan's algorithm (optimizer/hazan.nim:141). */
int32_t nfm_rng_rand_uniform(uint64_t* state, int64_t n, double max, double* out /*n*/);

#ifdef __cplusplus
}
#endif
#endif
