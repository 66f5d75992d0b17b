## hip_psgd.nim -- INCLUDED by nimfm's optimizer/psgd.nim (`when defined(nimfmHip): include hip_psgd`): PSGD keeps
## eta0 / scheduling / power / it / shuffle / nCalls private (optimizer/psgd.nim:16-20).  Overload of
## fit(self: PSGD[L, R], X, y, sfm, callback = nil) (:76-215) for nimfm_hip.HipCSRDataset: the per-sample step with the
## regulariser's lazy hooks (l1.nim:80-136, l21.nim:64-113), the cache resets and finalize (:58-73) run on the device; the
## epoch loop, the shuffle (Nim's global RNG, :120), the nCalls split (:179-182), the callbacks, the stopping rule (:198-201)
## and the verbose lines stay here.
## reg: newL1() or newL21().  newPSGD()'s default, newSquaredL12(), and newSquaredL21() are refused (their step touches every
## parameter per sample: newMBPSGD has their proximal operators), and so are OmegaTI and OmegaCS (no SGD hooks).
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip

proc psgdRegId(reg: L1): int32 = 0
proc psgdRegId(reg: L21): int32 = 1
proc psgdRegId[R](reg: R): int32 =
  raise newException(ValueError, "PSGD on the device takes newL1() or newL21(): the step of SquaredL12 / SquaredL21 touches " &
                                 "every parameter per sample (use newMBPSGD), OmegaTI and OmegaCS have no SGD hooks")

proc fit*[L, R](self: PSGD[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (PSGD[L, R], FactorizationMachine)->void = nil) =
  let reg = psgdRegId(self.reg)
  if sfm.P.shape[1] > 128:
    raise newException(ValueError, "PSGD on the device supports nComponents <= 128: use newMBPSGD(reg = newL1()) or newSGD")
  sfm.init(X)
  var yy = sfm.checkTarget(y)
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  if not sfm.warmStart: self.it = 1                               # :106-107
  let nSamples = X.nSamples
  let m = push(sfm, sfm.P.shape[2] - sfm.nAugments)
  var cfg = NfmMbpsgdCfg(eta0: self.eta0, alpha0: self.alpha0, alpha: self.alpha, beta: self.beta, gamma: self.gamma,
                         power: self.power, lossParam: lossParam(self.loss), loss: lossId(self.loss),
                         scheduling: ord(self.scheduling).int32, reg: reg, regTranspose: 0, batch: 1)
  var o: NfmOpt
  check nfm_psgd_create(m, addr cfg, addr o)
  try:
    check nfm_opt_set_it(o, self.it.int64)
    check nfm_psgd_begin_fit(o, X.handle)                         # reg.initSGD, :112
    if self.verbose > 0: echoHeader(self.maxIter, viol=false)
    var indices = toSeq(0..<nSamples)
    var isConverged = false
    var runningLossOld = 0.0
    for epoch in 0..<self.maxIter:
      var runningLoss = 0.0
      if self.shuffle: shuffle(indices)                           # :120
      let perm = if self.shuffle: cast[ptr int64](addr indices[0]) else: nil
      if not callback.isNil and self.nCalls > 0:
        var pos = 0
        while pos < nSamples:                                     # :179-182: it mod nCalls == 0, before inc(self.it)
          let toNext = (self.nCalls - self.it mod self.nCalls) mod self.nCalls + 1
          let last = min(nSamples, pos + toNext)
          var lossSum, viol: float64
          check nfm_opt_epoch(o, X.handle, perm, pos.int64, last.int64, addr lossSum, addr viol)
          runningLoss += lossSum
          self.it += last - pos
          pos = last
          if (self.it - 1) mod self.nCalls == 0:
            check nfm_psgd_finalize(o)
            pull(sfm, m)
            dec(self.it)
            callback(self, sfm)
            inc(self.it)
      else:
        var viol: float64
        check nfm_opt_epoch(o, X.handle, perm, 0, nSamples.int64, addr runningLoss, addr viol)
        self.it += nSamples
      runningLoss /= float(nSamples)                              # :186
      if not callback.isNil and self.nCalls <= 0:                 # :190-192
        check nfm_psgd_finalize(o)
        pull(sfm, m)
        callback(self, sfm)
      if runningLoss.classify == fcNan:                           # :194-196
        echo("Loss is NaN. Use smaller learning rate.")
        break
      if abs(runningLoss - runningLossOld) < self.tol:            # :198-201
        if self.verbose > 0: echo("Converged at epoch ", epoch, ".")
        isConverged = true
        break
      if self.verbose > 0:                                        # :203-207, on the working values: no finalize here
        pull(sfm, m)
        var regVal = regularization(sfm.P, sfm.w, sfm.intercept, self.alpha0, self.alpha, self.beta)
        for order in 0..<sfm.P.shape[0]:
          regVal += self.gamma * self.reg.eval(sfm.P[order].T, sfm.degree-order)
        echoInfo(epoch+1, self.maxIter, -1, runningLoss, regVal)
      runningLossOld = runningLoss
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    check nfm_psgd_finalize(o)                                    # :215
    pull(sfm, m)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)
