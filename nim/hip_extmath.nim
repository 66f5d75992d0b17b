## hip_extmath.nim -- INCLUDED by nimfm_hip.nim (`when defined(nimfmHip): include hip_extmath`): the sparse x dense products of
## extmath.nim on the device datasets, under the reference's names and argument order (include/nimfm_hip.h:
## nfm_dataset_matmul_sd, nfm_dataset_matmul_ds, nfm_dataset_mvmul, nfm_dataset_vmmul; DESIGN.md section 35).
##
##     matmul(D, S): Matrix    extmath.nim:10-37, 70-73    [m x nFeatures]
##     matmul(S, D): Matrix    extmath.nim:40-67, 76-79    [nSamples x r]
##     mvmul(S, vec): Vector   extmath.nim:82-101, 126-128
##     vmmul(vec, S): Vector   extmath.nim:104-123, 131-133
##
## S is a HipCSRDataset or a HipCSCDataset; every element has the bits of the reference's loops on the dataset type it stands
## for (the library reads the handle's layout).  The ValueErrors of a shape mismatch come from the library with the
## reference's texts.  A Matrix keeps one seq per row (tensor/tensor.nim:11-13), so the dense operand and the result cross the
## boundary through a flat row-major copy.  matmul(D, S) and vmmul of a HipCSRDataset make its column structure for the call:
## keep a HipCSCDataset (toCSCDataset) to repeat them.  norm (extmath.nim:136-163) has no device counterpart: normalize covers
## the norms of a resident dataset.
##
## NOTE: not compiled in the build image (no Nim toolchain); tests/test_gpu_extmath.py holds the library's side.

proc flatOf(D: Matrix): seq[float64] =
  result = newSeq[float64](D.shape[0] * D.shape[1])
  for i in 0..<D.shape[0]:
    for j in 0..<D.shape[1]:
      result[i * D.shape[1] + j] = D[i, j]

proc matrixOf(flat: seq[float64], rows, cols: int): Matrix =
  result = zeros([rows, cols])
  for i in 0..<rows:
    for j in 0..<cols:
      result[i, j] = flat[i * cols + j]

proc firstOf(s: var seq[float64]): ptr float64 = (if s.len > 0: addr s[0] else: nil)

proc matmul*(S: HipCSRDataset, D: Matrix): Matrix =
  var flat = flatOf(D)
  var res = newSeq[float64](S.nSamples * D.shape[1])
  check nfm_dataset_matmul_sd(S.handle, firstOf(flat), D.shape[0].int64, D.shape[1].int64, firstOf(res))
  result = matrixOf(res, S.nSamples, D.shape[1])

proc matmul*(D: Matrix, S: HipCSRDataset): Matrix =
  var flat = flatOf(D)
  var res = newSeq[float64](D.shape[0] * S.nFeaturesStored)
  check nfm_dataset_matmul_ds(S.handle, firstOf(flat), D.shape[0].int64, D.shape[1].int64, firstOf(res))
  result = matrixOf(res, D.shape[0], S.nFeaturesStored)

proc mvmul*(S: HipCSRDataset, vec: Vector): Vector =
  var v = vec
  result = zeros([S.nSamples])
  check nfm_dataset_mvmul(S.handle, firstOf(v), len(vec).int64, firstOf(result))

proc vmmul*(vec: Vector, S: HipCSRDataset): Vector =
  var v = vec
  result = zeros([S.nFeaturesStored])
  check nfm_dataset_vmmul(S.handle, firstOf(v), len(vec).int64, firstOf(result))

proc matmul*(S: HipCSCDataset, D: Matrix): Matrix = matmul(rowsOf(S), D)
proc matmul*(D: Matrix, S: HipCSCDataset): Matrix = matmul(D, rowsOf(S))
proc mvmul*(S: HipCSCDataset, vec: Vector): Vector = mvmul(rowsOf(S), vec)
proc vmmul*(vec: Vector, S: HipCSCDataset): Vector = vmmul(vec, rowsOf(S))
