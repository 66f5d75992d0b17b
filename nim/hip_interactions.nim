## hip_interactions.nim -- INCLUDED by nimfm_hip.nim (`when defined(nimfmHip): include hip_interactions`): which feature
## interactions a fitted FactorizationMachine uses (include/nimfm_hip.h: nfm_model_interaction_stats,
## nfm_model_top_interactions; DESIGN.md section 36).
##
##     interactionStats(fm, order)       what benchmarks/ml100k/sparse_fm*.nim print last, of W = P[order].T diag(lams) P[order]:
##                                       the L1 norm, the used interactions, the used features -- W is never stored
##     topInteractions(fm, K, order)     the K pairs i < j with W_ij != 0 by descending |W_ij|, then i, then j
##
## benchmarks/ml100k/utils.nim forms matmul(P.T, P) on the host ("Too slow"); here the rows of P.T that are not all zero
## are compacted and the product is reduced tile by tile on the device.  Field-aware and convex models are refused.

type InteractionStats* = tuple[l1Norm, l1OffDiag: float64, nInteractions, nFeatures, nNonzeroRows: int]

proc interactionStats*(self: FactorizationMachine, order: int = 0): InteractionStats =
  self.checkInitialized()
  let m = push(self, self.P.shape[2] - self.nAugments)
  var l1: array[2, float64]
  var counts: array[3, int64]
  let rc = nfm_model_interaction_stats(m, order.int32, addr l1[0], addr counts[0])
  discard nfm_model_destroy(m)
  check rc
  result = (l1[0], l1[1], counts[0].int, counts[1].int, counts[2].int)

proc topInteractions*(self: FactorizationMachine, K: int, order: int = 0): tuple[pairs: seq[array[2, int]], weights: seq[float64]] =
  ## 1 <= K <= 256; ranks that no used pair fills: pairs = [-1, -1], weights = NaN
  self.checkInitialized()
  let m = push(self, self.P.shape[2] - self.nAugments)
  let n = (if K >= 1 and K <= 256: K else: 0)   # out of range: the library refuses before it writes
  var pairs = newSeq[int64](2 * n)
  result.weights = newSeq[float64](n)
  let rc = nfm_model_top_interactions(m, order.int32, K.int64, (if n > 0: addr pairs[0] else: nil),
                                      (if n > 0: addr result.weights[0] else: nil))
  discard nfm_model_destroy(m)
  check rc
  result.pairs = newSeq[array[2, int]](n)
  for r in 0..<n: result.pairs[r] = [pairs[2 * r].int, pairs[2 * r + 1].int]

proc countInteractions*(self: FactorizationMachine, order: int = 0): int =
  ## benchmarks/ml100k/utils.nim: countInteractions(fm.P[order].T)
  result = interactionStats(self, order).nInteractions

proc countFeatures*(self: FactorizationMachine, order: int = 0): int =
  ## benchmarks/ml100k/utils.nim: countFeatures(fm.P[order].T)
  result = interactionStats(self, order).nFeatures
