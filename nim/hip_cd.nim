## hip_cd.nim -- INCLUDED by nimfm's optimizer/cd.nim (`when defined(nimfmHip): include hip_cd`):
## overload of fit(self: CD[L], X, y, fm, callback = nil) (optimizer/cd.nim:128-186) for nimfm_hip.HipCSRDataset.
## The reference fits a ColDataset; here the library builds the column twin of the row dataset itself (once per dataset,
## with the level schedule of DESIGN.md section 12), and the caches (yPred, cacheDeg2 / A, colNormSq) and every iteration
## run on the device.  The iteration loop, the stopping rule (:185-188), the verbose lines (:176-184) and the callback
## stay here.
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip

proc fit*[L](self: CD[L], X: HipCSRDataset, y: seq[float64], fm: FactorizationMachine,
             callback: (CD[L], FactorizationMachine)->void = nil) =
  fm.init(X)
  var yy = fm.checkTarget(y)
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nSamples = X.nSamples
  let m = push(fm, fm.P.shape[2] - fm.nAugments)
  var o: NfmOpt
  check nfm_cd_create(m, self.alpha0, self.alpha, self.beta, lossId(self.loss), lossParam(self.loss), addr o)
  var isConverged = false
  try:
    check nfm_cd_begin_fit(o, X.handle)                           # :128-153
    if self.verbose > 0: echoHeader(self.maxIter)
    for it in 0..<self.maxIter:                                   # :155-188
      var lossSum, viol: float64
      check nfm_opt_epoch(o, X.handle, nil, 0, nSamples.int64, addr lossSum, addr viol)
      if not callback.isNil:
        pull(fm, m)
        callback(self, fm)
      if self.verbose > 0:
        pull(fm, m)
        let n = float(nSamples)
        let reg = regularization(fm.P, fm.w, fm.intercept, self.alpha0 * n, self.alpha * n, self.beta * n) / n
        echoInfo(it+1, self.maxIter, viol, lossSum / n, reg)
      if viol < self.tol:
        if self.verbose > 0: echo("Converged at iteration ", it+1, ".")
        isConverged = true
        break
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pull(fm, m)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)

proc fit*[L](self: CD[L], X: HipCSCDataset, y: seq[float64], fm: FactorizationMachine,
             callback: (CD[L], FactorizationMachine)->void = nil) =
  ## optimizer/cd.nim:128 takes a ColDataset: the column-major device dataset, on its row twin (DESIGN.md section 25) --
  ## bit-equal to fit(self, toCSRDataset(X), y, fm, callback)
  fit(self, rowsOf(X), y, fm, callback)
