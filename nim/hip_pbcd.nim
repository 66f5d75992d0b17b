## hip_pbcd.nim -- INCLUDED by nimfm's optimizer/pbcd.nim (`when defined(nimfmHip): include hip_pbcd`):
## overload of fit(self: PBCD[L, R], X, y, sfm, callback = nil) (optimizer/pbcd.nim:212-329) for nimfm_hip.HipCSRDataset.
## A feature's whole row of P steps at once on the device: L1 and L21 on CD's level schedule, SquaredL21 (newPBCD's
## default) and OmegaCS (any degree) on the run schedule (DESIGN.md section 14).  maxSearch = 0 only (the reference's command line never sets another
## value) and the cyclic order only; shrink is stored and never read, here as there.  beta and gamma are NOT scaled by
## nSamples (:138,147,154).  The iteration loop, the stopping rule (:316-320) and the verbose lines (:302-307, BEFORE the
## callback, :309-314) stay here.  The file is included, so the private fields of PBCD (maxSearch, shuffle) are in reach.
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
# pbcd.nim itself imports only newSquaredL21 from the regularisers; the overloads below need the types
import ../regularizer/regularizers

proc pbcdRegId(reg: L1): int32 = 0
proc pbcdRegId(reg: L21): int32 = 1
proc pbcdRegId(reg: SquaredL21): int32 = 3
proc pbcdRegId(reg: OmegaCS): int32 = 5

proc fit*[L, R](self: PBCD[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (PBCD[L, R], FactorizationMachine)->void = nil) =
  if self.maxSearch != 0:
    raise newException(ValueError, "maxSearch != 0 (the line search, pbcd.nim:80-109) is not supported on the device.")
  if self.shuffle:
    raise newException(ValueError, "shuffle=true is not supported on the device.")
  sfm.init(X)
  var yy = sfm.checkTarget(y)
  # initBCD (:271): SquaredL21 raises for degree != 2 and for transpose = true; OmegaCS's host copy is not read again
  self.reg.initBCD(sfm.degree, X.nFeatures + sfm.nAugments, sfm.P.shape[1])
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nSamples = X.nSamples
  let m = push(sfm, sfm.P.shape[2] - sfm.nAugments)
  var o: NfmOpt
  check nfm_pbcd_create(m, self.alpha0, self.alpha, self.beta, self.gamma, lossId(self.loss), lossParam(self.loss),
                        pbcdRegId(self.reg), int32(self.maxSearch), addr o)
  var isConverged = false
  try:
    check nfm_cd_begin_fit(o, X.handle)                           # :232-271
    if self.verbose > 0: echoHeader(self.maxIter)
    for it in 0..<self.maxIter:                                   # :275-320
      var lossSum, viol: float64
      check nfm_opt_epoch(o, X.handle, nil, 0, nSamples.int64, addr lossSum, addr viol)
      if self.verbose > 0:
        pull(sfm, m)
        var regVal = regularization(sfm.P, sfm.w, sfm.intercept, self.alpha0, self.alpha, self.beta)  # :303-306, unscaled
        for order in 0..<sfm.P.shape[0]:
          regVal += self.gamma * self.reg.eval(sfm.P[order].T, sfm.degree-order)
        echoInfo(it+1, self.maxIter, viol, lossSum / float(nSamples), regVal)
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

proc fit*[L, R](self: PBCD[L, R], X: HipCSCDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (PBCD[L, R], FactorizationMachine)->void = nil) =
  ## optimizer/pbcd.nim:212 takes a ColDataset: the column-major device dataset, on its row twin (DESIGN.md section 25)
  fit(self, rowsOf(X), y, sfm, callback)
