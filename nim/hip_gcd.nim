## hip_gcd.nim -- INCLUDED by nimfm's optimizer/greedy_cd.nim (`when defined(nimfmHip): include hip_gcd`): GreedyCD keeps
## maxIterInner / maxIterPower / nRefitting / refitFully / tolPower private (optimizer/greedy_cd.nim:8-22).  An overload of
## fit(self: GreedyCD[L], X, y, cfm, callback = nil) (:415-500) for nimfm_hip.HipCSRDataset at refitFully = false.  yPred, dL, K,
## P, lams, w, colNormSq and the power method's vectors stay in the library for the whole fit (nfm_gcd_create / nfm_gcd_begin_fit /
## nfm_gcd_outer_begin / one nfm_gcd_inner per inner iteration / nfm_gcd_outer_end, DESIGN.md section 21); the outer and the
## inner loop, both stopping tests, the refit schedule, the verbose lines, the callback and the draw of the power method's start
## vector from Nim's global generator (tensor/tensor.nim:920-921) stay here.  The vector is drawn only in the inner iterations
## that add a base (nComponents < maxComponents), so that randomize(1); fit consumes the stream as the reference does.
## refitFully = true (ADMM, Newton-CG, two dsyev calls) stays with the reference: the library answers NFM_ERR_UNSUPPORTED and
## fit raises ValueError.  pushConvex / pullConvex are hip_hazan.nim's.
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
import random, strutils, strformat
from hazan import pushConvex, pullConvex

proc fit*[L](self: GreedyCD[L], X: HipCSRDataset, y: seq[float64], cfm: ConvexFactorizationMachine,
             callback: (GreedyCD[L], ConvexFactorizationMachine)->void = nil) =
  if self.nRefitting < 1:
    raise newException(ValueError, "nRefitting < 1.")             # :384 would divide by zero
  cfm.init(X)
  var yy = cfm.checkTarget(y)
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nFeatures = X.nFeaturesStored
  let m = pushConvex(cfm, nFeatures)
  var o: NfmOpt
  check nfm_gcd_create(m, self.alpha0, self.alpha, self.beta, lossId(self.loss), lossParam(self.loss), self.maxIterPower.int64,
                       self.tolPower, self.refitFully.int32, addr o)
  try:
    var oldLossVal, oldRegVal, newLossVal, newRegVal: float64
    let rc = nfm_gcd_begin_fit(o, X.handle, addr oldLossVal, addr oldRegVal)   # :419-457
    if rc == -5 and self.refitFully:                              # NFM_ERR_UNSUPPORTED: refitFully = true is refused here
      raise newException(ValueError, $nfm_last_error())
    check rc
    var isConverged = false
    var start = newSeq[float64](nFeatures)
    var rec: array[8, float64]                                    # NFM_GCD_REC_*
    for it in 0..<self.maxIter:
      if self.verbose > 0:
        echo(fmt"Outer Iteration {it+1}")
      check nfm_gcd_outer_begin(o, X.handle, addr rec[0])         # :464-469 and fitZ's head :332-336
      var nComponents = rec[5].int
      var oldObj = rec[6]
      for itIn in 0..<self.maxIterInner:                          # fitZ, :347-412
        let addBase = nComponents < cfm.maxComponents
        if addBase:
          for j in 0..<nFeatures: start[j] = 2*rand(1.0) - 1.0    # the global generator, only when a base is added
        let refit = (itIn+1) mod self.nRefitting == 0
        check nfm_gcd_inner(o, X.handle, (if addBase: addr start[0] else: nil), refit.int32, addr rec[0])
        nComponents = rec[5].int
        if rec[0] != 0.0 or refit or itIn == self.maxIterInner-1: # :392
          let newObj = rec[6]
          if self.verbose > 1:
            let iterAligned = align($(itIn+1), len($self.maxIterInner))
            stdout.write(fmt"   Iteration: {iterAligned}")
            stdout.write(fmt"   Objective: {newObj:1.4e}")
            stdout.write(fmt"   Decreasing: {oldObj - newObj:1.4e}")
            stdout.write("\n")
            stdout.flushFile()
          if abs(newObj - oldObj) < self.tol:
            if self.verbose > 1:
              echo("   Converged at iteration ", itIn+1, ".")
            break
          oldObj = newObj
      # :474-476; yPred is rebuilt (:493-497) when another outer iteration may follow: nothing reads it before that
      check nfm_gcd_outer_end(o, X.handle, (it < self.maxIter - 1).int32, addr newLossVal, addr newRegVal)
      if not callback.isNil:                                      # :478-479
        pullConvex(cfm, m, nFeatures)
        callback(self, cfm)
      if self.verbose > 0:
        stdout.write(fmt"   Loss: {newLossVal:1.4e}")
        stdout.write(fmt"   Reg: {newRegVal:1.4e}")
        stdout.write("\n")
      if abs(newLossVal + newRegVal - oldLossVal - oldRegVal) < self.tol:
        if self.verbose > 0:
          echo("Converged at iteration ", it+1, ".")
        isConverged = true
        break
      oldLossVal = newLossVal
      oldRegVal = newRegVal
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pullConvex(cfm, m, nFeatures)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)

proc fit*[L](self: GreedyCD[L], X: HipCSCDataset, y: seq[float64], cfm: ConvexFactorizationMachine,
             callback: (GreedyCD[L], ConvexFactorizationMachine)->void = nil) =
  ## optimizer/greedy_cd.nim's fit takes a ColDataset: the column-major device dataset, on its row twin (DESIGN.md section 25)
  fit(self, rowsOf(X), y, cfm, callback)
