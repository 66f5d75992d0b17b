## hip_pcd.nim -- INCLUDED by nimfm's optimizer/pcd.nim (`when defined(nimfmHip): include hip_pcd`):
## overload of fit(self: PCD[L, R], X, y, sfm, callback = nil) (optimizer/pcd.nim:110-201) for nimfm_hip.HipCSRDataset.
## CD's device iteration with a proximal step per feature: L1 and row-wise SquaredL12 on the level schedule, column-wise
## SquaredL12 (newSquaredL12()'s default) and OmegaTI on the run schedule (DESIGN.md section 13).  The iteration loop, the
## stopping rule (:194-197), the verbose lines (:176-189, BEFORE the callback, :191-192) stay here.
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
# pcd.nim itself imports only newSquaredL12 from the regularisers; the overloads below need the types
import ../regularizer/regularizers

proc pcdRegId(reg: L1): int32 = 0
proc pcdRegId(reg: SquaredL12): int32 = 2
proc pcdRegId(reg: OmegaTI): int32 = 4

# The layout of the penalty.  SquaredL12.transpose is private (squaredl12.nim:7) and this file sits in another module,
# so it is derived from the exported eval (squaredl12.nim:72-75): on a 2 x 1 matrix of ones the column-wise penalty
# (transpose = true) is (1 + 1)^2 = 4, the row-wise one 1^2 + 1^2 = 2.  L1 and OmegaTI have no layout.
proc pcdRegTranspose(reg: L1): int32 = 0
proc pcdRegTranspose(reg: OmegaTI): int32 = 0
proc pcdRegTranspose(reg: SquaredL12): int32 =
  if reg.eval(ones([2, 1])) > 3.0: 1 else: 0

proc fit*[L, R](self: PCD[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (PCD[L, R], FactorizationMachine)->void = nil) =
  sfm.init(X)
  var yy = sfm.checkTarget(y)
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nSamples = X.nSamples
  let m = push(sfm, sfm.P.shape[2] - sfm.nAugments)
  var o: NfmOpt
  check nfm_pcd_create(m, self.alpha0, self.alpha, self.beta, self.gamma, lossId(self.loss), lossParam(self.loss),
                       pcdRegId(self.reg), pcdRegTranspose(self.reg), addr o)
  var isConverged = false
  try:
    check nfm_cd_begin_fit(o, X.handle)                           # :128-154
    if self.verbose > 0: echoHeader(self.maxIter)
    for it in 0..<self.maxIter:                                   # :156-197
      var lossSum, viol: float64
      check nfm_opt_epoch(o, X.handle, nil, 0, nSamples.int64, addr lossSum, addr viol)
      if self.verbose > 0:
        pull(sfm, m)
        let n = float(nSamples)
        var regVal = 0.0
        for order in 0..<sfm.P.shape[0]:
          regVal += self.gamma * n * self.reg.eval(sfm.P[order].T, sfm.degree-order)
        regVal += regularization(sfm.P, sfm.w, sfm.intercept, self.alpha0 * n, self.alpha * n, self.beta * n)
        echoInfo(it+1, self.maxIter, viol, lossSum / n, regVal / n)
      if not callback.isNil:
        pull(sfm, m)
        callback(self, sfm)
      if viol < self.tol:
        if self.verbose > 0: echo("Converged at iteration ", it+1, ".")
        isConverged = true
        break
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pull(sfm, m)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)

proc fit*[L, R](self: PCD[L, R], X: HipCSCDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (PCD[L, R], FactorizationMachine)->void = nil) =
  ## optimizer/pcd.nim:110 takes a ColDataset: the column-major device dataset, on its row twin (DESIGN.md section 25)
  fit(self, rowsOf(X), y, sfm, callback)
