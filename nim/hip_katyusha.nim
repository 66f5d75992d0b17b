## hip_katyusha.nim -- INCLUDED by nimfm's optimizer/katyusha.nim (`when defined(nimfmHip): include hip_katyusha`): Katyusha
## keeps eta / miniBatchSize / shuffle / tau1 / tau2 / nCalls private (optimizer/katyusha.nim:12-21).  Overload of
## fit(self: Katyusha[L, R], X, y, sfm, callback = nil) (:156-269) for nimfm_hip.HipCSRDataset.  The seven parameter sets, the
## variance-reduced mini-batch gradient and the dense updates of the inner loop run in the library (nfm_katyusha_create /
## nfm_katyusha_begin_fit / one nfm_opt_epoch per outer iteration, DESIGN.md section 16); the index stream (indices[ii] with
## wrap-around and reshuffle, :108-118), the stopping test on viol, the per-epoch callback and the verbose lines stay here.
## After every outer iteration the model handle holds what finalize (:56-73) gives the user.  nCalls > 0 (a callback inside
## the inner loop) is refused; beta <= 0, alpha <= 0 with fitLinear, alpha0 <= 0 with fitIntercept and eta <= 0 are refused
## by nfm_katyusha_create (ValueError) where the reference returns NaN parameters.
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
import ../regularizer/regularizers

proc katRegId(reg: L1): int32 = 0
proc katRegId(reg: L21): int32 = 1
proc katRegId(reg: SquaredL12): int32 = 2
proc katRegId(reg: SquaredL21): int32 = 3
proc katTranspose(reg: L1): int32 = 0
proc katTranspose(reg: L21): int32 = 0
proc katTranspose(reg: SquaredL12): int32 = int32(reg.transpose)
proc katTranspose(reg: SquaredL21): int32 = int32(reg.transpose)

proc fit*[L, R](self: Katyusha[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                callback: (Katyusha[L, R], FactorizationMachine)->void = nil) =
  if self.nCalls > 0:
    raise newException(ValueError, "Katyusha: nCalls > 0 (a callback inside the inner loop) is not supported; nCalls <= 0 calls the callback once per epoch")
  sfm.init(X)
  var yy = sfm.checkTarget(y)
  # initSGD (katyusha.nim:219): SquaredL12 / SquaredL21 raise for degree != 2
  self.reg.initSGD(sfm.degree, X.nFeatures + sfm.nAugments, sfm.P.shape[1])
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nSamples = X.nSamples
  var B = self.miniBatchSize
  if B <= 0: B = max((X.nFeatures * nSamples) div X.nnz, 1)       # :203-206
  let inner = (nSamples-1) div B + 1                              # :207
  let m = push(sfm, sfm.P.shape[2] - sfm.nAugments)
  var o: NfmOpt
  check nfm_katyusha_create(m, self.eta, self.alpha0, self.alpha, self.beta, self.gamma, self.tau1, self.tau2,
                            lossId(self.loss), lossParam(self.loss), katRegId(self.reg), katTranspose(self.reg), B.int64, addr o)
  var indices = toSeq(0..<nSamples)
  var stream = newSeq[int](B * inner)
  var ii = 0
  if self.shuffle: shuffle(indices)                               # :199-200
  var isConverged = false
  try:
    check nfm_katyusha_begin_fit(o, X.handle)
    if self.verbose > 0:
      echo("Minibatch size: ", B)
      echo("Number of inner iteration: ", inner)
      echoHeader(self.maxIter, viol=true)
    var tilde = newParams(sfm.P.shape, sfm.w.len, sfm.fitLinear, sfm.fitIntercept)
    tilde.P = zeros([sfm.P.shape[0], sfm.P.shape[2], sfm.P.shape[1]])
    for it in 0..<self.maxIter:
      for q in 0..<stream.len:                                    # :108-118: indices[ii], wrap and reshuffle
        stream[q] = indices[ii]
        inc(ii)
        if ii >= nSamples:
          ii = 0
          if self.shuffle: shuffle(indices)
      var lossSum, viol: float64
      check nfm_opt_epoch(o, X.handle, cast[ptr int64](addr stream[0]), 0, stream.len.int64, addr lossSum, addr viol)
      if not callback.isNil:                                      # :237-239: the finalized model
        pull(sfm, m)
        callback(self, sfm)
      let lossVal = lossSum / float(nSamples)                     # :241-244: the loss at the snapshot the epoch started from
      if lossVal.classify == fcNan:
        echo("Loss is NaN. Use smaller learning rate.")
        break
      if self.verbose > 0:                                        # :249-253: regVal on tilde
        check nfm_katyusha_snapshot(o, addr tilde.P.data[0], addr tilde.w[0], addr tilde.intercept)
        var regVal = regularization(tilde, self.alpha0, self.alpha, self.beta)
        for order in 0..<tilde.P.shape[0]:
          regVal += self.gamma * self.reg.eval(tilde.P[order], sfm.degree-order)
        echoInfo(it+1, self.maxIter, viol, lossVal, regVal)
      if viol < self.tol:
        if self.verbose > 0: echo("Converged at epoch ", it+1, ".")
        isConverged = true
        break
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pull(sfm, m)                                                  # :269: finalize's model, already in the handle
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)
