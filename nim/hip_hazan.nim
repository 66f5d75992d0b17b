## hip_hazan.nim -- INCLUDED by nimfm's optimizer/hazan.nim (`when defined(nimfmHip): include hip_hazan`): Hazan keeps eta /
## maxIterPower / tolPower / optimal / nTol / it private (optimizer/hazan.nim:8-19).  Overloads of
## fit(self: Hazan, X, y, cfm, callback = nil) (:59-225) and of decisionFunction(self: ConvexFactorizationMachine, X)
## (model/convex_factorization_machine.nim:63-84) for nimfm_hip.HipCSRDataset.  yPredLinear, yPredQuad, the residual, K, P,
## lams, w, colNormSq and the vectors of the power method and of CG stay in the library for the whole fit (nfm_hazan_create /
## nfm_hazan_begin_fit / one nfm_hazan_iter per outer iteration, DESIGN.md section 20); the outer loop, the nTol stopping rule,
## the verbose line, the callback and the draw of the power method's start vector from Nim's global generator
## (tensor/tensor.nim:920-921) stay here.  The library's cg ends after 1000 iterations and when curv is 0 or not finite; the
## reference's has no working cap (tensor/tensor.nim:992).
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
import random, strutils, strformat

proc flatRows(P: Matrix): seq[float64] =
  result = newSeqOfCap[float64](P.shape[0] * P.shape[1])
  for s in 0..<P.shape[0]:
    for j in 0..<P.shape[1]: result.add(P[s, j])

proc pushConvex*(cfm: ConvexFactorizationMachine, nFeatures: int): NfmModel =
  ## the model handle of the convex kind, holding cfm's current basis (P.shape[0] of maxComponents slots in use)
  check nfm_cfm_create(hipContext(), (if cfm.task == classification: 1 else: 0).int32, cfm.maxComponents.int32,
                       cfm.fitIntercept.int32, cfm.fitLinear.int32, cfm.ignoreDiag.int32, nFeatures.int64, addr result)
  var P = flatRows(cfm.P)
  var lams = cfm.lams
  var w = cfm.w
  check nfm_cfm_set_params(result, cfm.P.shape[0].int32, (if P.len > 0: addr P[0] else: nil),
                           (if lams.len > 0: addr lams[0] else: nil), addr w[0], cfm.intercept)

proc pullConvex*(cfm: ConvexFactorizationMachine, m: NfmModel, nFeatures: int) =
  ## P [nComponents][nFeatures], lams, w and the intercept back from the handle
  var nc: int32
  var P = newSeq[float64](cfm.maxComponents * nFeatures)
  var lams = newSeq[float64](cfm.maxComponents)
  check nfm_cfm_get_params(m, addr nc, addr P[0], addr lams[0], addr cfm.w[0], addr cfm.intercept)
  cfm.P = zeros([nc.int, nFeatures])
  cfm.lams = zeros([nc.int])
  for s in 0..<nc.int:
    cfm.lams[s] = lams[s]
    for j in 0..<nFeatures: cfm.P[s, j] = P[s * nFeatures + j]

proc decisionFunction*(self: ConvexFactorizationMachine, X: HipCSRDataset): seq[float64] =
  ## model/convex_factorization_machine.nim:63-84 on a device-resident dataset
  self.checkInitialized()
  if X.nFeaturesStored != self.P.shape[1]:
    raise newException(ValueError, "Invalid nFeatures.")          # :76-77
  let m = pushConvex(self, X.nFeaturesStored)
  result = newSeq[float64](X.nSamples)
  if X.nSamples > 0: check nfm_decision_function(m, X.handle, addr result[0])
  discard nfm_model_destroy(m)

proc fit*(self: Hazan, X: HipCSRDataset, y: seq[float64], cfm: ConvexFactorizationMachine,
          callback: (Hazan, ConvexFactorizationMachine)->void = nil) =
  cfm.init(X)
  var yy = cfm.checkTarget(y)
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nFeatures = X.nFeaturesStored
  let m = pushConvex(cfm, nFeatures)
  var o: NfmOpt
  check nfm_hazan_create(m, self.eta, self.maxIterPower.int64, self.tolPower, self.optimal.int32, addr o)
  try:
    var lossOld: float64
    check nfm_hazan_begin_fit(o, X.handle, addr lossOld)
    if not cfm.warmStart: self.it = 0                             # :87-88
    var nComponents = cfm.P.shape[0]
    var nTol = 0
    var isConverged = false
    var start = newSeq[float64](nFeatures)
    var rec: array[8, float64]                                    # NFM_HAZAN_REC_*
    for it in 0..<self.maxIter:
      if not self.optimal and nComponents >= cfm.maxComponents:   # :137-138
        break
      for j in 0..<nFeatures: start[j] = 2*rand(1.0) - 1.0        # tensor/tensor.nim:920-921, the global generator
      check nfm_hazan_iter(o, X.handle, self.it.int64, addr start[0], addr rec[0])
      nComponents = rec[7].int
      if not callback.isNil:                                      # :198-199
        pullConvex(cfm, m, nFeatures)
        callback(self, cfm)
      let lossNew = rec[0]
      if self.verbose > 0:                                        # :203-209
        let epochAligned = align($(self.it), len($self.maxIter))
        stdout.write(fmt"Epoch: {epochAligned}")
        stdout.write(fmt"   MSE/2: {lossNew/2.0:1.4e}")
        stdout.write(fmt"   Trace Norm: {rec[1]:1.4e}")
        stdout.write("\n")
      if lossOld - lossNew < self.tol:                            # :211-219
        inc(nTol)
        if nTol >= self.nTol:
          if self.verbose > 0: echo("Converged at iteration ", self.it+1, ".")
          isConverged = true
          break
      else:
        nTol = 0
      lossOld = lossNew
      inc(self.it)
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pullConvex(cfm, m, nFeatures)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)

proc decisionFunction*(self: ConvexFactorizationMachine, X: HipCSCDataset): seq[float64] =
  ## model/convex_factorization_machine.nim:63-84 for the column-major device dataset (its row twin)
  result = decisionFunction(self, rowsOf(X))

proc fit*(self: Hazan, X: HipCSCDataset, y: seq[float64], cfm: ConvexFactorizationMachine,
          callback: (Hazan, ConvexFactorizationMachine)->void = nil) =
  ## optimizer/hazan.nim's fit takes a ColDataset: the column-major device dataset, on its row twin (DESIGN.md section 25)
  fit(self, rowsOf(X), y, cfm, callback)
