## hip_cross.nim -- INCLUDED by nimfm_hip.nim (`when defined(nimfmHip): include hip_cross`): every pair of two row sets scored
## by a degree-2 FactorizationMachine, and the topK items of every user, on the device datasets (include/nimfm_hip.h:
## nfm_cross_decision_function, nfm_cross_topk, nfm_cross_rank_of, nfm_cross_pairs, nfm_cross_topk_among, nfm_sample_candidates;
## DESIGN.md section 32).
##
##     crossDecisionFunction(fm, U, V)[i][j]   decisionFunction (model/factorization_machine.nim:100-122, kernels.nim:59-64) of
##                                             row i of U followed by row j of V -- row i * nV + j of hstack(U[rep], V[tile])
##                                             (tensor/sparse.nim:671-698), which is never made
##     recommend(fm, U, V, topK)               per user the topK (item, score) by descending score, then ascending item; the
##                                             scores are crossDecisionFunction's bit for bit
##
##     recommend(fm, U, V, seen, topK)         the same over the items a user has not seen: a stored entry (i, j) of seen
##                                             takes item j out of user i's candidates (ids = -1, scores = NaN past the last)
##     rankingScore(fm, U, V, heldOut, topK)   precision, recall, ndcg and hit rate of those lists against heldOut, on the device
##     rankOf(fm, U, V, heldOut, seen)         the place of every held-out item in the user's full list, counted without a list
##
##     crossDecisionFunctionAt(fm, U, V, pairs)      the scores of the stored entries of pairs [nU x nV] alone, the same bits
##     recommendAmong(fm, U, V, topK, candidates)    recommend over the items stored in the user's row of candidates
##     rankingScoreAmong(fm, U, V, heldOut, topK, candidates)   rankingScore of those lists
##     sampleCandidates(exclude, nPerUser, seed, includeSet)    the candidates drawn on the device: per user nPerUser items stored
##                                                              in neither matrix, and every item of includeSet
##
## The reference has none of them: it scores the rows it is given.  Everything but a FactorizationMachine of degree 2 on resident
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

proc recommendImpl(self: FactorizationMachine, U, V: HipCSRDataset, topK: int, chunkItems: int,
                   seen: HipCSRDataset = nil): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  let K = (if topK >= 1 and topK <= 256: topK else: 0)   # out of range: the library refuses before it writes
  var ids = newSeq[int64](U.nSamples * K)
  var scores = newSeq[float64](U.nSamples * K)
  let pIds = (if ids.len > 0: addr ids[0] else: nil)
  let pScores = (if scores.len > 0: addr scores[0] else: nil)
  let rc = (if seen.isNil: nfm_cross_topk(m, U.handle, V.handle, topK.int64, chunkItems.int64, pIds, pScores)
            else: nfm_cross_topk_seen(m, U.handle, V.handle, seen.handle, topK.int64, chunkItems.int64, pIds, pScores))
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

proc recommend*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, seen: HipCSRDataset, topK: int,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  ## over the items a user has not seen: a stored entry (i, j) of seen [nU x nV] takes item j out of user i's candidates,
  ## whatever its value; ranks that no candidate fills are ids = -1, scores = NaN (column-major sets: pass rowsOf(X))
  result = recommendImpl(self, U, V, topK, chunkItems, seen)

type RankingScore* = tuple[precision, recall, ndcg, hitRate: float64, nUsers: int]

proc rankingScore*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, heldOut: HipCSRDataset, topK: int,
                   seen: HipCSRDataset = nil, chunkItems: int = 0): RankingScore =
  ## precision, recall, ndcg and hit rate at topK of recommend's lists against heldOut [nU x nV] (distinct ids inside a row),
  ## each the mean over the nUsers users whose held-out row is not empty; computed on the device
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  var o: array[5, float64]
  let rc = nfm_cross_rank_metrics(m, U.handle, V.handle, (if seen.isNil: NfmDataset(nil) else: seen.handle), heldOut.handle,
                                  topK.int64, chunkItems.int64, addr o[0])
  discard nfm_model_destroy(m)
  check rc
  result = (o[0], o[1], o[2], o[3], o[4].int)

proc rankOf*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, heldOut: HipCSRDataset, seen: HipCSRDataset = nil,
             chunkItems: int = 0): tuple[ranks: seq[int], nCandidates: seq[int]] =
  ## ranks[e], for the stored entry e = (i, j) of heldOut [nU x nV] in storage order: how many items j' != j not stored in row i
  ## of seen rank before j for user i (descending score, then ascending id, NaN last) -- j's place in the full list, no topK; -1
  ## where j itself is stored in row i of seen.  nCandidates[i]: nV minus the distinct ids of row i of seen.  Counted on the
  ## device without a list (column-major sets: pass rowsOf(X))
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  var nnz: int64
  var ranks: seq[int64]
  var cand = newSeq[int64](U.nSamples)
  var rc = nfm_dataset_shape(heldOut.handle, nil, nil, addr nnz, nil)
  if rc == 0:
    ranks = newSeq[int64](nnz.int)
    rc = nfm_cross_rank_of(m, U.handle, V.handle, heldOut.handle, (if seen.isNil: NfmDataset(nil) else: seen.handle), chunkItems.int64,
                           (if ranks.len > 0: addr ranks[0] else: nil), (if cand.len > 0: addr cand[0] else: nil))
  discard nfm_model_destroy(m)
  check rc
  result.ranks = newSeq[int](ranks.len)
  for e in 0..<ranks.len: result.ranks[e] = ranks[e].int
  result.nCandidates = newSeq[int](cand.len)
  for i in 0..<cand.len: result.nCandidates[i] = cand[i].int

proc crossDecisionFunctionAt*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, pairs: HipCSRDataset): seq[float64] =
  ## the scores of the stored entries of pairs [nU x nV], in storage order: [e] has exactly the bits of
  ## crossDecisionFunction(U, V)[i][j] for the pair (i, j) of entry e, and only those pairs are computed (column-major sets:
  ## pass rowsOf(X))
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  var nnz: int64
  var rc = nfm_dataset_shape(pairs.handle, nil, nil, addr nnz, nil)
  if rc == 0:
    result = newSeq[float64](nnz.int)
    rc = nfm_cross_pairs(m, U.handle, V.handle, pairs.handle, (if result.len > 0: addr result[0] else: nil))
  discard nfm_model_destroy(m)
  check rc

proc recommendAmong*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, topK: int,
                     candidates: HipCSRDataset): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  ## recommend over the items stored in the user's row of candidates [nU x nV] (a repeated id counts once): the lists of
  ## recommend(U, V, seen = the complement of candidates, topK) byte for byte, scoring the candidates alone
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  let K = (if topK >= 1 and topK <= 256: topK else: 0)
  var ids = newSeq[int64](U.nSamples * K)
  var scores = newSeq[float64](U.nSamples * K)
  let rc = nfm_cross_topk_among(m, U.handle, V.handle, candidates.handle, topK.int64, (if ids.len > 0: addr ids[0] else: nil),
                                (if scores.len > 0: addr scores[0] else: nil))
  discard nfm_model_destroy(m)
  check rc
  result.ids = newSeq[seq[int]](U.nSamples)
  result.scores = newSeq[seq[float64]](U.nSamples)
  for i in 0..<U.nSamples:
    result.ids[i] = newSeq[int](K)
    for r in 0..<K: result.ids[i][r] = ids[i * K + r].int
    result.scores[i] = scores[i * K ..< (i + 1) * K]

proc rankingScoreAmong*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset, heldOut: HipCSRDataset, topK: int,
                        candidates: HipCSRDataset): RankingScore =
  ## rankingScore of recommendAmong's lists, which never leave the device
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")
  let m = push(self, U.nFeaturesStored + V.nFeaturesStored)
  var o: array[5, float64]
  let rc = nfm_cross_rank_metrics_among(m, U.handle, V.handle, candidates.handle, heldOut.handle, topK.int64, addr o[0])
  discard nfm_model_destroy(m)
  check rc
  result = (o[0], o[1], o[2], o[3], o[4].int)

proc sampleCandidates*(exclude: HipCSRDataset, nPerUser: int, seed: uint64, includeSet: HipCSRDataset = nil): HipCSRDataset =
  ## a new resident dataset [nU x nV], values 1.0, rows ascending and distinct: per user min(nPerUser, eligible) items drawn
  ## uniformly without replacement from the items stored neither in the user's row of exclude nor of includeSet, and every item
  ## of the user's row of includeSet (`include` is a Nim keyword) -- what recommendAmong and rankingScoreAmong read in place.  A
  ## pure function of its arguments (include/nimfm_hip.h: nfm_sample_candidates); 1 <= nPerUser <= 1024; column-major sets pass
  ## rowsOf(X)
  var h: NfmDataset
  check nfm_sample_candidates(exclude.handle, (if includeSet.isNil: nil else: includeSet.handle), nPerUser.int64, cast[int64](seed), addr h)
  result = adopt(h)
