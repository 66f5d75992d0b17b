## hip_dataset.nim -- the reference's dataset procs on the device datasets, under the reference's names (include/nimfm_hip.h,
## DESIGN.md section 23).  Included by nimfm_hip.nim (INTEGRATION.md): it needs no private field of nimfm's objects.
##
##     X[indicesRow], X[a..<b], X[a..^b]   dataset.nim:319-369
##     shuffle(X, y[, indices])            dataset.nim:372-395
##     vstack / hstack                     tensor/sparse.nim:564-581, 613-633 / :671-698, 719-750
##     normalize(X, axis, norm)            dataset.nim:398-403 (in place: the object takes the new handle)
##     loadUserItemRatingFile(f, X, y)     dataset.nim:840-900
##     dumpSVMLightFile / dumpFFMFile      dataset.nim:793-805, 825-837 (DESIGN.md section 24)
##
## and, at the end of the file, the column-major dataset HipCSCDataset (DESIGN.md section 25) with
##
##     toHip(CSCDataset), toCSCDataset, toCSRDataset      dataset.nim:124-129, tensor/sparse.nim:510-527, 490-507
##     loadSVMLightFile / loadUserItemRatingFile as CSC   dataset.nim:643-693, 903-992
##     X[a..<b], X[a..^b], vstack, hstack, normalize      tensor/sparse.nim:300-330, 583-610, 701-716, 414-427
##
## HipCSRDataset and HipCSRFieldDataset are one object type, so every overload below serves both; the library refuses a
## stack that mixes the kinds.  Every result is a new dataset resident in HBM; the inputs are never modified (normalize swaps
## the handle inside X and destroys the old one).  A dataset used in row blocks (nfm_stream_*) has no handle of this kind and
## no overload here.
##
## NOTE: not compiled in the build image (no Nim toolchain); tests/test_dataset_ops_shim.py holds the calls to the header.

proc `[]`*(X: ref HipDatasetObj, indicesRow: openarray[int]): ref HipDatasetObj =
  ## dataset.nim:319-326, 353-359; checkIndicesRow's ValueErrors come from the library with the reference's texts
  var h: NfmDataset
  check nfm_dataset_select_rows(X.handle, (if indicesRow.len > 0: cast[ptr int64](unsafeAddr indicesRow[0]) else: nil),
                                indicesRow.len.int64, addr h)
  result = adopt(h)
  result.nAugments = X.nAugments

proc `[]`*(X: ref HipDatasetObj, slice: Slice[int]): ref HipDatasetObj =
  ## dataset.nim:328-330, 362-364: X[a..b] = X[toSeq(a..b)], a contiguous piece of every array
  var h: NfmDataset
  check nfm_dataset_slice_rows(X.handle, slice.a.int64, (slice.b + 1).int64, addr h)
  result = adopt(h)
  result.nAugments = X.nAugments

proc `[]`*(X: ref HipDatasetObj, slice: HSlice[int, BackwardsIndex]): ref HipDatasetObj =
  ## dataset.nim:333-335, 367-369
  result = X[slice.a..(X.nSamples - int(slice.b))]

proc shuffle*[U](X: ref HipDatasetObj, y: seq[U], indices: openarray[int]): (ref HipDatasetObj, seq[U]) =
  ## dataset.nim:372-381
  if len(y) != X.nSamples:
    raise newException(ValueError, "X.nSamples != len(y)")
  let Xs = X[indices]  # checkIndicesRow before y is read, as X[indices] raises first in the reference's result tuple
  var yShuffled = newSeq[U](len(indices))
  for ii, i in indices:
    yShuffled[ii] = y[i]
  result = (Xs, yShuffled)

proc shuffle*[U](X: ref HipDatasetObj, y: seq[U]): (ref HipDatasetObj, seq[U]) =
  ## dataset.nim:384-395: the forward draw from Nim's global generator (nfm_rng_shuffle_forward is the same procedure for
  ## hosts without it)
  if len(y) != X.nSamples:
    raise newException(ValueError, "X.nSamples != len(y)")
  var indices = toSeq(0..<len(y))
  var j, tmp: int
  for i in 0..<len(y):
    j = rand(len(y)-1-i)
    tmp = indices[i]
    indices[i] = indices[i+j]
    indices[i+j] = tmp
  result = shuffle(X, y, indices)

proc stackHandles(dataseq: openarray[ref HipDatasetObj]): seq[NfmDataset] =
  if dataseq.len < 1:
    raise newException(ValueError, "no datasets to stack")
  for X in dataseq: result.add(X.handle)

proc vstack*(dataseq: varargs[ref HipDatasetObj]): ref HipDatasetObj =
  ## tensor/sparse.nim:564-581, 613-633: "All matrics must have the same shape[1]."
  var hs = stackHandles(dataseq)
  var h: NfmDataset
  check nfm_dataset_vstack(addr hs[0], hs.len.int64, addr h)
  result = adopt(h)
  result.nAugments = dataseq[0].nAugments

proc hstack*(dataseq: varargs[ref HipDatasetObj]): ref HipDatasetObj =
  ## tensor/sparse.nim:671-698, 719-750: "All matrics must have the same shape[0]."
  var hs = stackHandles(dataseq)
  var h: NfmDataset
  check nfm_dataset_hstack(addr hs[0], hs.len.int64, addr h)
  result = adopt(h)
  result.nAugments = dataseq[0].nAugments

proc normalize*(X: ref HipDatasetObj, axis = 1, norm: NormKind = l2) =
  ## dataset.nim:398-403: in place -- X takes the normalised copy's handle, the old arrays are freed.  ord(norm) is the
  ## library's NFM_NORM_* (tensor/sparse.nim:37-38).  Augmented features play no part: the device dataset stores none.
  var h: NfmDataset
  check nfm_dataset_normalize(X.handle, axis.int32, ord(norm).int32, addr h)
  discard nfm_dataset_destroy(X.handle)
  X.handle = h

proc loadUserItemRatingFile*(f: string, X: var HipCSRDataset, y: var seq[float64]) =
  ## dataset.nim:840-900, same signature with the device dataset type: the text is parsed on the GPU
  var h: NfmDataset
  check nfm_dataset_load_user_item(hipContext(), f.cstring, addr h)
  X = adopt(h)
  y = targets(X)

proc dumpTargets[U](X: ref HipDatasetObj, y: seq[U]): seq[float64] =
  ## dataset.nim:796, 828
  if X.nSamples != len(y):
    raise newException(ValueError, "X.nSamples != len(y).")
  result = newSeq[float64](len(y))
  for i, v in y: result[i] = float64(v)

proc dumpSVMLightFile*(f: string, X: HipCSRDataset, y: seq[float64]) =
  ## dataset.nim:793-805 with the device dataset type: the text is formatted on the GPU (DESIGN.md section 24), the same
  ## bytes as the reference writes from the host
  var yd = dumpTargets(X, y)
  check nfm_dataset_dump_svmlight(X.handle, f.cstring, (if yd.len > 0: addr yd[0] else: nil), 0'i32, 0'i64)

proc dumpSVMLightFile*(f: string, X: HipCSRDataset, y: seq[int]) =
  ## the reference's `f.write(y[i])` for y: seq[int]: the targets are written as integers
  var yd = dumpTargets(X, y)
  check nfm_dataset_dump_svmlight(X.handle, f.cstring, (if yd.len > 0: addr yd[0] else: nil), 1'i32, 0'i64)

proc dumpFFMFile*(f: string, X: HipCSRFieldDataset, y: seq[float64]) =
  ## dataset.nim:825-837; HipCSRDataset and HipCSRFieldDataset are one object type: the library refuses the wrong kind
  var yd = dumpTargets(X, y)
  check nfm_dataset_dump_ffm(X.handle, f.cstring, (if yd.len > 0: addr yd[0] else: nil), 0'i32, 0'i64)

proc dumpFFMFile*(f: string, X: HipCSRFieldDataset, y: seq[int]) =
  var yd = dumpTargets(X, y)
  check nfm_dataset_dump_ffm(X.handle, f.cstring, (if yd.len > 0: addr yd[0] else: nil), 1'i32, 0'i64)

proc formatText*(X: ref HipDatasetObj): string =
  ## the bytes dumpSVMLightFile / dumpFFMFile would write with the dataset's own targets
  var n: int64
  check nfm_dataset_format_text(X.handle, nil, 0'i32, 0'i64, nil, 0'i64, addr n)
  result = newString(n.int)
  if n > 0:
    check nfm_dataset_format_text(X.handle, nil, 0'i32, 0'i64, result.cstring, n, addr n)

# ---------------------------------------------------------------------------------------------------------
# column-major datasets (DESIGN.md section 25)
# ---------------------------------------------------------------------------------------------------------
type
  HipCSCDataset* = distinct HipCSRDataset  ## BaseDataset[CSCMatrix] in HBM (dataset.nim:18-22): a handle whose layout is
                                           ## NFM_LAYOUT_CSC.  A distinct type, so what the reference compiles for a
                                           ## RowDataset only (SGD, AdaGrad, PSGD, X[indices], shuffle, the dumps) does not
                                           ## compile for it here either; the library refuses the handle as well.

proc rowsOf*(X: HipCSCDataset): HipCSRDataset = HipCSRDataset(X)
  ## the same handle under the row type: decisionFunction, score and the column-wise solvers run on its row twin, which the
  ## library made with the dataset

proc nSamples*(X: HipCSCDataset): int = rowsOf(X).nSamples
proc nnz*(X: HipCSCDataset): int = rowsOf(X).nnz
proc nFeatures*(X: HipCSCDataset): int = rowsOf(X).nFeatures
proc shape*(X: HipCSCDataset): array[2, int] = rowsOf(X).shape
proc nCached*(X: HipCSCDataset): int = rowsOf(X).nSamples

proc toHip*(X: CSCDataset): HipCSCDataset =
  ## newCSCDataset (dataset.nim:124-129) on the device; tensor/sparse.nim:14-17: data / indices / indptr of a CSCMatrix
  var h: NfmDataset
  let nnz = X.data.data.len
  check nfm_dataset_create_csc(hipContext(), X.nSamples.int64, X.data.shape[1].int64,
                               cast[ptr int64](unsafeAddr X.data.indptr[0]),
                               (if nnz > 0: cast[ptr int64](unsafeAddr X.data.indices[0]) else: nil),
                               (if nnz > 0: unsafeAddr X.data.data[0] else: nil), nil, addr h)
  result = HipCSCDataset(adopt(h))

proc toCSCDataset*(X: HipCSRDataset): HipCSCDataset =
  ## tensor/sparse.nim:510-527 on the device; the targets are carried over
  var h: NfmDataset
  check nfm_dataset_to_csc(X.handle, addr h)
  result = HipCSCDataset(adopt(h))
  rowsOf(result).nAugments = X.nAugments

proc toCSRDataset*(X: HipCSCDataset): HipCSRDataset =
  ## tensor/sparse.nim:490-507 on the device
  var h: NfmDataset
  check nfm_dataset_to_csr(rowsOf(X).handle, addr h)
  result = adopt(h)
  result.nAugments = rowsOf(X).nAugments

proc loadSVMLightFile*(f: string, dataset: var HipCSCDataset, y: var seq[float64], nFeatures: int = -1) =
  ## dataset.nim:643-693: the GPU parse of the row loader followed by the transposition
  var X: HipCSRDataset
  loadSVMLightFile(f, X, y, nFeatures)
  dataset = toCSCDataset(X)

proc loadUserItemRatingFile*(f: string, X: var HipCSCDataset, y: var seq[float64]) =
  ## dataset.nim:903-992: lines of fewer than 5 characters are skipped (:923, 955, 975)
  var h: NfmDataset
  check nfm_dataset_load_user_item_lines(hipContext(), f.cstring, 1'i32, addr h)
  let rows = adopt(h)
  y = targets(rows)
  X = toCSCDataset(rows)

proc `[]`*(X: HipCSCDataset, slice: Slice[int]): HipCSCDataset =
  ## tensor/sparse.nim:300-325
  var h: NfmDataset
  check nfm_dataset_slice_rows(rowsOf(X).handle, slice.a.int64, (slice.b + 1).int64, addr h)
  result = HipCSCDataset(adopt(h))
  rowsOf(result).nAugments = rowsOf(X).nAugments

proc `[]`*(X: HipCSCDataset, slice: HSlice[int, BackwardsIndex]): HipCSCDataset =
  ## tensor/sparse.nim:328-330
  result = X[slice.a..(X.nSamples - int(slice.b))]

proc cscHandles(dataseq: openarray[HipCSCDataset]): seq[NfmDataset] =
  if dataseq.len < 1:
    raise newException(ValueError, "no datasets to stack")
  for X in dataseq: result.add(rowsOf(X).handle)

proc vstack*(dataseq: varargs[HipCSCDataset]): HipCSCDataset =
  ## tensor/sparse.nim:583-610; the result's indptr has nFeatures + 1 entries (the reference: shape[0] + 1, :598)
  var hs = cscHandles(dataseq)
  var h: NfmDataset
  check nfm_dataset_vstack(addr hs[0], hs.len.int64, addr h)
  result = HipCSCDataset(adopt(h))

proc hstack*(dataseq: varargs[HipCSCDataset]): HipCSCDataset =
  ## tensor/sparse.nim:701-716: "All matrics must have the same shape[0]"
  var hs = cscHandles(dataseq)
  var h: NfmDataset
  check nfm_dataset_hstack(addr hs[0], hs.len.int64, addr h)
  result = HipCSCDataset(adopt(h))

proc normalize*(X: HipCSCDataset, axis = 1, norm: NormKind = l2) =
  ## tensor/sparse.nim:414-427, in place
  normalize(rowsOf(X), axis, norm)

proc decisionFunction*(self: FactorizationMachine, X: HipCSCDataset): seq[float64] =
  ## model/factorization_machine.nim:100-122 for a ColDataset: the column walk adds a sample's terms by ascending column id
  ## (kernels.nim:4-44), the storage order of the row twin
  result = decisionFunction(self, rowsOf(X))

# ---------------------------------------------------------------------------------------------------------
# the binary stream files, written and transposed on the device (DESIGN.md section 30)
# ---------------------------------------------------------------------------------------------------------
proc newHipStreamCSCDataset*(f: string, fY: string = ""): HipCSCDataset =
  ## dataset.nim:176-179 newStreamCSCDataset: the STREAMCSC file becomes a column-major dataset resident in HBM; fY: the
  ## raw float64 labels (loadStreamLabel, :1007-1014) become its targets
  var h: NfmDataset
  check nfm_dataset_load_stream_csc(hipContext(), f.cstring, (if fY.len > 0: fY.cstring else: nil), addr h)
  result = HipCSCDataset(adopt(h))

proc dumpStreamFile*(f: string, X: HipCSRDataset) =
  ## X as a STREAMCSR file (field-aware: STREAMCSRFIELD), packed on the GPU: what newHipStreamCSRDataset reloads
  check nfm_dataset_dump_stream(X.handle, f.cstring, 0'i64)

proc dumpStreamFile*(f: string, X: HipCSCDataset) =
  ## X as a STREAMCSC file: what newHipStreamCSCDataset reloads
  check nfm_dataset_dump_stream(rowsOf(X).handle, f.cstring, 0'i64)

# transposeFile and convertFFMFile have no overload here: they take only strings, so a proc of either name would be ambiguous
# with the reference's own (dataset.nim:1100, 1202) wherever both modules are seen.  A host that wants the device versions calls
# nfm_transpose_file / nfm_convert_ffm (nimfm_hip.nim) with hipContext().
