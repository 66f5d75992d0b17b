## hip_cross.nim -- INCLUDED by nimfm_hip.nim (`when defined(nimfmHip): include hip_cross`): every pair of two row sets scored
## by a degree-2 FactorizationMachine, and the topK items of every user, on the device datasets (include/nimfm_hip.h:
## nfm_cross_decision_function, nfm_cross_topk; DESIGN.md section 32).
##
##     crossDecisionFunction(fm, U, V)[i][j]   decisionFunction (model/factorization_machine.nim:100-122, kernels.nim:59-64) of
##                                             row i of U followed by row j of V -- row i * nV + j of hstack(U[rep], V[tile])
##                                             (tensor/sparse.nim:671-698), which is never made
##     recommend(fm, U, V, topK)               per user the topK (item, score) by descending score, then ascending item; the
##                                             scores are crossDecisionFunction's bit for bit
##
## The reference has neither: it scores the rows it is given.  Everything but a FactorizationMachine of degree 2 on resident
## datasets is refused by the library with a message that names the pairs and decisionFunction as the way that remains.

proc crossImpl(self: FactorizationMachine, U, V: HipCSRDataset): seq[seq[float64]] =
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")   # factorization_machine.nim:114-115
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  var flat = newSeq[float64](U.nSamples * V.nSamples)
  let rc = nfm_cross_decision_function(m, U.handle, V.handle, (if flat.len > 0: addr flat[0] else: nil))
  discard nfm_model_destroy(m)
  check rc
  result = newSeq[seq[float64]](U.nSamples)
  for i in 0..<U.nSamples:
    result[i] = flat[i * V.nSamples ..< (i + 1) * V.nSamples]

proc recommendImpl(self: FactorizationMachine, U, V: HipCSRDataset, topK: int,
                   chunkItems: int): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  let K = (if topK >= 1 and topK <= 256: topK else: 0)   # out of range: the library refuses before it writes
  var ids = newSeq[int64](U.nSamples * K)
  var scores = newSeq[float64](U.nSamples * K)
  let rc = nfm_cross_topk(m, U.handle, V.handle, topK.int64, chunkItems.int64, (if ids.len > 0: addr ids[0] else: nil),
                          (if scores.len > 0: addr scores[0] else: nil))
  discard nfm_model_destroy(m)
  check rc
  result.ids = newSeq[seq[int]](U.nSamples)
  result.scores = newSeq[seq[float64]](U.nSamples)
  for i in 0..<U.nSamples:
    result.ids[i] = newSeq[int](K)
    for r in 0..<K: result.ids[i][r] = ids[i * K + r].int
    result.scores[i] = scores[i * K ..< (i + 1) * K]

proc crossDecisionFunction*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset): seq[seq[float64]] =
  ## [nU][nV]
  result = crossImpl(self, U, V)

proc crossDecisionFunction*(self: FactorizationMachine, U: HipCSCDataset, V: HipCSCDataset): seq[seq[float64]] =
  ## column-major sets are read through their row twins, as decisionFunction reads them
  result = crossImpl(self, rowsOf(U), rowsOf(V))

proc crossDecisionFunction*(self: FactorizationMachine, U: HipCSCDataset, V: HipCSRDataset): seq[seq[float64]] =
  result = crossImpl(self, rowsOf(U), V)

proc crossDecisionFunction*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSCDataset): seq[seq[float64]] =
  result = crossImpl(self, U, rowsOf(V))

proc recommend*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, topK: int,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  ## 1 <= topK <= min(nV, 256); chunkItems: the items one workgroup ranks, 0 = the library's choice (the result does not
  ## depend on it)
  result = recommendImpl(self, U, V, topK, chunkItems)

proc recommend*(self: FactorizationMachine, U: HipCSCDataset, V: HipCSCDataset, topK: int,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  result = recommendImpl(self, rowsOf(U), rowsOf(V), topK, chunkItems)

proc recommend*(self: FactorizationMachine, U: HipCSCDataset, V: HipCSRDataset, topK: int,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  result = recommendImpl(self, rowsOf(U), V, topK, chunkItems)

proc recommend*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSCDataset, topK: int,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  result = recommendImpl(self, U, rowsOf(V), topK, chunkItems)
