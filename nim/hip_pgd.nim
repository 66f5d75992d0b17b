## hip_pgd.nim -- INCLUDED by nimfm's optimizer/pgd.nim, fista.nim and nmapgd.nim (`when defined(nimfmHip): include hip_pgd`):
## overloads of fit(self: PGD[L, R] / FISTA[L, R] / NMAPGD[L, R], X, y, sfm, callback = nil) (optimizer/pgd.nim:149-217,
## fista.nim:52-141, nmapgd.nim:174-268) for nimfm_hip.HipCSRDataset.  The algorithm -- gradient, line search, FISTA's accept /
## restart, NMAPGD's Z / V -- runs in the library with every parameter set resident on the device (nfm_pgd_create /
## nfm_pgd_begin_fit / one nfm_opt_epoch per iteration, DESIGN.md section 15).  The iteration loop, the stopping test on the
## SQUARED distance, the callback (BEFORE the verbose line) and the verbose lines stay here.  The file is included, so the
## private fields (rho, sigma, maxSearch, NMAPGD's eta) are in reach; each module gets the overload of the type it declares.
## The device optimizer is made per fit: a warm-started model's t (and NMAPGD's c, q, caches) live on a handle, so a Nim
## host that fits the same model repeatedly keeps the handle instead (nfm_pgd_begin_fit's warm_start).
## Not compiled in the build image (no Nim toolchain); see nimfm_hip.nim.
import nimfm_hip
import ../regularizer/regularizers

proc pgdRegId(reg: L1): int32 = 0
proc pgdRegId(reg: L21): int32 = 1
proc pgdRegId(reg: SquaredL12): int32 = 2
proc pgdRegId(reg: SquaredL21): int32 = 3
proc pgdTranspose(reg: L1): int32 = 0
proc pgdTranspose(reg: L21): int32 = 0
proc pgdTranspose(reg: SquaredL12): int32 = int32(reg.transpose)
proc pgdTranspose(reg: SquaredL21): int32 = int32(reg.transpose)

template hipPgdFit(self, algo, etaNm, labelOffset, X, y, sfm, callback: untyped) =
  sfm.init(X)
  var yy = sfm.checkTarget(y)
  # initSGD (pgd.nim:180): SquaredL12 / SquaredL21 raise for degree != 2
  self.reg.initSGD(sfm.degree, X.nFeatures + sfm.nAugments, sfm.P.shape[1])
  check nfm_dataset_set_targets(X.handle, addr yy[0])
  let nSamples = X.nSamples
  let m = push(sfm, sfm.P.shape[2] - sfm.nAugments)
  var o: NfmOpt
  check nfm_pgd_create(m, int32(algo), self.alpha0, self.alpha, self.beta, self.gamma, self.rho, self.sigma, etaNm,
                       lossId(self.loss), lossParam(self.loss), pgdRegId(self.reg), pgdTranspose(self.reg),
                       int64(self.maxSearch), addr o)
  var isConverged = false
  try:
    check nfm_pgd_begin_fit(o, X.handle, int32(sfm.warmStart))
    if self.verbose > 0: echoHeader(self.maxIter, viol=true)
    for it in 0..<self.maxIter:
      var lossSum, viol: float64
      var rec: array[13, float64]                                  # NFM_PGD_IT_COUNT
      check nfm_opt_epoch(o, X.handle, nil, 0, nSamples.int64, addr lossSum, addr viol)
      check nfm_pgd_last_iter(o, addr rec[0])
      if not callback.isNil:                                       # finalize, then the callback
        pull(sfm, m)
        callback(self, sfm)
      if self.verbose > 0:
        echoInfo(it+1, self.maxIter, viol, rec[0], rec[1])         # lossVal, regVal
      if viol < self.tol:
        if self.verbose > 0: echo("Converged at epoch ", it + labelOffset, ".")
        isConverged = true
        break
    if not isConverged and self.verbose > 0:
      echo("Objective did not converge. Increase maxIter.")
    pull(sfm, m)
  finally:
    discard nfm_opt_destroy(o)
    discard nfm_model_destroy(m)

when declared(PGD):
  proc fit*[L, R](self: PGD[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                  callback: (PGD[L, R], FactorizationMachine)->void = nil) =
    hipPgdFit(self, 0, 0.5, 0, X, y, sfm, callback)                # pgd.nim:209 prints `epoch`, not `epoch+1`

when declared(FISTA):
  proc fit*[L, R](self: FISTA[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                  callback: (FISTA[L, R], FactorizationMachine)->void = nil) =
    hipPgdFit(self, 1, 0.5, 1, X, y, sfm, callback)

when declared(NMAPGD):
  proc fit*[L, R](self: NMAPGD[L, R], X: HipCSRDataset, y: seq[float64], sfm: FactorizationMachine,
                  callback: (NMAPGD[L, R], FactorizationMachine)->void = nil) =
    hipPgdFit(self, 2, self.eta, 1, X, y, sfm, callback)           # alpha0 already holds alpha (nmapgd.nim:44)
