## hip_ranker.nim -- INCLUDED by nimfm_hip.nim (`when defined(nimfmHip): include hip_ranker`): the Ranker, the resident sides
## of one (model, U, V) (include/nimfm_hip.h: nfm_ranker_create, nfm_ranker_destroy, nfm_ranker_scores, nfm_ranker_scores_at,
## nfm_ranker_topk, nfm_ranker_rank_of; DESIGN.md section 34).
##
##     newRanker(fm, U, V)     a FactorizationMachine of degree 2: the sides crossDecisionFunction makes per call, kept
##     newRanker(ffm, U, V)    a FieldAwareFactorizationMachine on field datasets: [i][j] is decisionFunction
##                             (model/field_aware_factorization_machine.nim:52-76) of row i of U followed by row j of V with its
##                             columns moved up by U's nFeatures and its fields by U's nFields (tensor/sparse.nim:719-750)
##     scores(r)               [nU][nV]
##     scoresAt(r, pairs)      the stored entries of pairs [nU x nV], the same bits
##     recommend(r, topK, seen)      per user the topK (item, score) by descending score, then ascending item
##     rankOf(r, heldOut, seen)      the place of every held-out item in the user's full list
##
## The ranker is a snapshot of the model's parameters when it is made: a later fit does not change it.  The reference has no
## counterpart: it scores the rows it is given.  What the library refuses names the pairs and decisionFunction as the way that
## remains.  Column-major sets pass rowsOf(X).

type
  RankerObj = object
    handle: pointer
    nUsers*, nItems*: int
  Ranker* = ref RankerObj

proc release(r: Ranker) =
  if not r.handle.isNil:
    discard nfm_ranker_destroy(r.handle)
    r.handle = nil

proc rankerOf(m: NfmModel, U, V: ref HipDatasetObj): Ranker =
  new(result, release)
  let rc = nfm_ranker_create(m, U.handle, V.handle, addr result.handle)
  discard nfm_model_destroy(m)
  check rc
  (result.nUsers, result.nItems) = (U.nSamples, V.nSamples)

proc newRanker*(self: FactorizationMachine, U: HipCSRDataset, V: HipCSRDataset): Ranker =
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored + self.nAugments != self.P.shape[2]:
    raise newException(ValueError, "Invalid nFeatures.")   # factorization_machine.nim:114-115
  result = rankerOf(push(self, U.nFeaturesStored + V.nFeaturesStored), U, V)

proc newRanker*(self: FieldAwareFactorizationMachine, U: HipCSRFieldDataset, V: HipCSRFieldDataset): Ranker =
  self.checkInitialized()
  if U.nFeaturesStored + V.nFeaturesStored != self.P.shape[1]: raise newException(ValueError, "Invalid nFeatures.")
  if U.nFields + V.nFields != self.P.shape[0]: raise newException(ValueError, "Invalid nFields.")   # :63-64
  result = rankerOf(push(self), U, V)

proc scores*(self: Ranker): seq[seq[float64]] =
  ## [nUsers][nItems]
  var flat = newSeq[float64](self.nUsers * self.nItems)
  check nfm_ranker_scores(self.handle, (if flat.len > 0: addr flat[0] else: nil))
  result = newSeq[seq[float64]](self.nUsers)
  for i in 0..<self.nUsers:
    result[i] = flat[i * self.nItems ..< (i + 1) * self.nItems]

proc scoresAt*(self: Ranker, pairs: HipCSRDataset): seq[float64] =
  ## the scores of the stored entries of pairs [nUsers x nItems] in storage order: exactly the bits of scores()[i][j]
  result = newSeq[float64](pairs.nnz)
  check nfm_ranker_scores_at(self.handle, pairs.handle, (if result.len > 0: addr result[0] else: nil))

proc recommend*(self: Ranker, topK: int, seen: HipCSRDataset = nil,
                chunkItems: int = 0): tuple[ids: seq[seq[int]], scores: seq[seq[float64]]] =
  ## 1 <= topK <= min(nItems, 256); a stored entry (i, j) of seen takes item j out of user i's candidates (ids = -1, scores =
  ## NaN past the last candidate); the result does not depend on chunkItems
  let K = (if topK >= 1 and topK <= 256: topK else: 0)   # out of range: the library refuses before it writes
  var ids = newSeq[int64](self.nUsers * K)
  var scores = newSeq[float64](self.nUsers * K)
  check nfm_ranker_topk(self.handle, topK.int64, (if seen.isNil: NfmDataset(nil) else: seen.handle), chunkItems.int64,
                        (if ids.len > 0: addr ids[0] else: nil), (if scores.len > 0: addr scores[0] else: nil))
  result.ids = newSeq[seq[int]](self.nUsers)
  result.scores = newSeq[seq[float64]](self.nUsers)
  for i in 0..<self.nUsers:
    result.ids[i] = newSeq[int](K)
    for r in 0..<K: result.ids[i][r] = ids[i * K + r].int
    result.scores[i] = scores[i * K ..< (i + 1) * K]

proc rankOf*(self: Ranker, heldOut: HipCSRDataset, seen: HipCSRDataset = nil,
             chunkItems: int = 0): tuple[ranks: seq[int], nCandidates: seq[int]] =
  ## ranks[e], for the stored entry e = (i, j) of heldOut in storage order: the unseen items that rank before j for user i; -1
  ## where j itself is stored in row i of seen.  nCandidates[i]: nItems minus the distinct ids of row i of seen
  var ranks = newSeq[int64](heldOut.nnz)
  var cand = newSeq[int64](self.nUsers)
  check nfm_ranker_rank_of(self.handle, heldOut.handle, (if seen.isNil: NfmDataset(nil) else: seen.handle), chunkItems.int64,
                           (if ranks.len > 0: addr ranks[0] else: nil), (if cand.len > 0: addr cand[0] else: nil))
  result.ranks = newSeq[int](ranks.len)
  for e in 0..<ranks.len: result.ranks[e] = ranks[e].int
  result.nCandidates = newSeq[int](cand.len)
  for i in 0..<cand.len: result.nCandidates[i] = cand[i].int
