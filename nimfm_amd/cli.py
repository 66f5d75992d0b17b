"""`python -m nimfm_amd train|test ...` -- the reference's end-user commands (`nimfm train`, `nimfm test`,
/root/reference/src/nimfm.nim:72-134) for the solvers that run on the MI355X path (`--solver sgd|adagrad`, plus `mbpsgd` from `nimfm_sparsefm`):
`--solver nmapgd|fista` are that command line's full-batch proximal gradient solvers (nimfm_sparsefm.nim:47-57);
svmlight files are parsed on the GPU (ingest.hip), training runs in libnimfm_hip.so, the test score is
reduced on the device, models are written/read in the reference's text format (`dump`/`load`,
model/factorization_machine.nim:142-220).  Option names follow the reference's proc parameters (cligen
accepts both `--nComponents` and `--n-components`; so does this parser).  The coordinate-descent solvers
(`cd`, `als`) are refused by this command line; coordinate descent itself runs on the device through the library's hosts
(`nimfm_amd.newCD(...).fit`, `CD<L>` in nimfm_amd/host/nimfm.hpp, nim/hip_cd.nim).
`--solver hazan` is `nimfm_cfm train --solver hazan` (src/nimfm_cfm.nim:35-104): a convex factorization machine fitted by Hazan's
algorithm, with that command line's `--maxComponents`, `--eta`, `--maxIterPower`, `--ignoreDiag` and `--optimal` and its defaults;
`test --load` reads a convex dump too (`--ignoreDiag` says which kernel: the dump does not store it).  `--solver gcd`, that command
line's greedy coordinate descent, is refused here and points to `nimfm_amd.newGreedyCD`, which runs it on the device.
`--solver psgd --reg l1|l21` is `newPSGD` (optimizer/psgd.nim) with `--gamma`, `--eta0`, `--scheduling` and `--power`; the other
`--reg` values are refused with a message that names `--solver mbpsgd`."""
import argparse
import sys

import numpy as np


def _both(name):
    """--nComponents and --n-components"""
    dashed = "".join("-" + c.lower() if c.isupper() else c for c in name)
    return ["--" + name] if dashed == name else ["--" + name, "--" + dashed]


def _flag(v):
    return str(v).lower() in ("1", "true", "yes", "y", "on")


def _parser():
    ap = argparse.ArgumentParser(prog="nimfm_amd", description="Factorization machines on an MI355X (nimfm's train / test).")
    sub = ap.add_subparsers(dest="cmd", required=True)
    tr = sub.add_parser("train", help="training a factorization machine")
    te = sub.add_parser("test", help="test a factorization machine")
    for p in (tr, te):
        p.add_argument("-t", "--task", required=True, help="r for regression and c for binary classification")
        p.add_argument("--loss", default="squared")
        p.add_argument("--dump", default="")
        p.add_argument("--predict", default="")
        p.add_argument(*_both("nFeatures"), dest="nFeatures", type=int, default=-1)
        p.add_argument("--verbose", type=int, default=1)
        # nimfm_cfm's model option (src/nimfm_cfm.nim:64-72); its dump does not store it, so `test --load` takes it too
        p.add_argument(*_both("ignoreDiag"), dest="ignoreDiag", default="false")
    tr.add_argument("--train", required=True)
    tr.add_argument("--test", default="")
    tr.add_argument("--degree", type=int, default=2)
    tr.add_argument(*_both("nComponents"), dest="nComponents", type=int, default=30)
    tr.add_argument("--alpha0", type=float, default=1e-7)
    tr.add_argument("--alpha", type=float, default=1e-5)
    tr.add_argument("--beta", type=float, default=1e-3)
    tr.add_argument(*_both("fitLower"), dest="fitLower", default="explicit")
    tr.add_argument(*_both("fitLinear"), dest="fitLinear", default="true")
    tr.add_argument(*_both("fitIntercept"), dest="fitIntercept", default="true")
    tr.add_argument("--scale", type=float, default=0.1)
    tr.add_argument(*_both("randomState"), dest="randomState", type=int, default=1)
    tr.add_argument("--solver", default="sgd",
                    help="sgd or adagrad; psgd = proximal SGD with the lazily updated --reg l1|l21 (optimizer/psgd.nim); "
                         "mbpsgd / pcd / nmapgd / fista / katyusha = the mini-batch proximal SGD, proximal coordinate "
                         "descent, full-batch proximal gradient and Katyusha solvers of the reference's nimfm_sparsefm CLI "
                         "(src/nimfm_sparsefm.nim:44-70); cd / als are not offered here "
                         "(nimfm_amd.newCD(...).fit)")
    # nimfm_sparsefm train's extra options (src/nimfm_sparsefm.nim:160-170), used by --solver mbpsgd and pcd
    tr.add_argument("--gamma", type=float, default=1e-5)
    tr.add_argument("--reg", default="squaredl12", help="l1, l21, squaredl12 or squaredl21 (pcd: l1 or squaredl12)")
    tr.add_argument(*_both("miniBatchSize"), dest="miniBatchSize", type=int, default=-1)
    tr.add_argument(*_both("maxIter"), dest="maxIter", type=int, default=100)
    tr.add_argument("--tol", type=float, default=1e-5)
    tr.add_argument("--eta0", type=float, default=0.1)
    tr.add_argument("--scheduling", default="optimal")
    tr.add_argument("--power", type=float, default=1.0)
    tr.add_argument("--threshold", type=float, default=0.1)
    tr.add_argument("--load", default="")
    # the line search of --solver nmapgd|fista (newNMAPGD / newFISTA's parameters; defaults: each solver's own)
    tr.add_argument("--rho", type=float, default=0.5)
    tr.add_argument("--sigma", type=float, default=None, help="nmapgd: 0.01, fista: 1.0")
    tr.add_argument(*_both("maxSearch"), dest="maxSearch", type=int, default=-1)
    # nimfm_cfm train's options (src/nimfm_cfm.nim:36-41,64-72), used by --solver hazan
    tr.add_argument(*_both("maxComponents"), dest="maxComponents", type=int, default=30)
    tr.add_argument("--eta", type=float, default=1000.0)
    tr.add_argument(*_both("maxIterPower"), dest="maxIterPower", type=int, default=100)
    tr.add_argument("--optimal", default="true")
    # this path's own knobs
    tr.add_argument("--mode", default="sequential", choices=["sequential", "minibatch"],
                    help="sequential = the reference's single-thread order; minibatch = the deterministic data-parallel rule")
    tr.add_argument("--batch", type=int, default=8192)
    tr.add_argument(*_both("touchCap"), dest="touchCap", default="1",
                    help="minibatch SGD: steps of a batch on one coordinate summed before averaging sets in (1: the mean; auto: "
                         "about twice the touches per coordinate and batch, nimfm_amd.suggestTouchCap)")
    tr.add_argument(*_both("adaCross"), dest="adaCross", type=float, default=0.0,
                    help="minibatch AdaGrad: weight of the batch's gradient cross products in g_norm (0.1 for large batches)")
    tr.add_argument("--shuffle", default="true")
    te.add_argument("--test", required=True)
    te.add_argument("--load", required=True)
    return ap


def _echo_data_info(X):
    """nimfm.nim:8-13"""
    _, _, data, _ = X.to_host()
    print("   Number of samples  : %d" % X.nSamples)
    print("   Number of features : %d" % X.nFeatures)
    print("   Number of non-zeros: %d" % X.nnz)
    print("   Maximum value      : %s" % (repr(float(data.max())) if len(data) else "-inf"))
    print("   Minimum value      : %s" % (repr(float(data.min())) if len(data) else "inf"))


def _eval(nf, fm, task, test, predict, n_features, verbose):
    """nimfm.nim:16-35; the score is reduced on the device"""
    if verbose > 0:
        print("Load test data")
    X, y = nf.loadSVMLightFile(test, n_features)
    if verbose > 0:
        _echo_data_info(X)
    score = fm.score(X, y)
    print(("Test RMSE: %r" if task == "regression" else "Test Accuracy: %r") % score)
    if predict:
        with open(predict, "w") as f:
            for v in fm.decisionFunction(X):
                f.write(repr(float(v)) + "\n")


def _train_hazan(nf, args, task):
    """nimfm_cfm train --solver hazan (src/nimfm_cfm.nim:35-104): squared loss only (optimizer/hazan.nim:9)"""
    if args.loss != "squared":
        raise ValueError("Hazan's algorithm fits the squared loss only (optimizer/hazan.nim:9), not %s" % args.loss)
    if args.load:
        cfm = nf.load(args.load, True, ignoreDiag=_flag(args.ignoreDiag))
        if not isinstance(cfm, nf.ConvexFactorizationMachine):
            raise ValueError("--solver hazan needs the dump of a convex factorization machine")
    else:
        cfm = nf.newConvexFactorizationMachine(task, maxComponents=args.maxComponents, ignoreDiag=_flag(args.ignoreDiag),
                                               fitIntercept=_flag(args.fitIntercept), fitLinear=_flag(args.fitLinear), warmStart=False)
    X, y = nf.loadSVMLightFile(args.train, args.nFeatures)
    if args.verbose > 0:
        _echo_data_info(X)
        _echo_data_info(X)  # nimfm_cfm.nim:46,56 print it twice for hazan
    opt = nf.newHazan(args.maxIter, eta=args.eta, maxIterPower=args.maxIterPower, optimal=_flag(args.optimal), verbose=args.verbose,
                      tol=args.tol)
    opt.fit(X, y, cfm)
    if args.test:
        _eval(nf, cfm, task, args.test, args.predict, args.nFeatures, args.verbose)
    if args.dump:
        cfm.dump(args.dump)
    return 0


def main(argv=None):
    args = _parser().parse_args(argv)
    import nimfm_amd as nf

    task = {"r": "regression", "c": "classification"}.get(args.task, args.task)
    if args.loss not in ("squared", "huber", "squared_hinge", "logistic"):
        raise ValueError("loss %s is not supported" % args.loss)
    if args.cmd == "test":
        fm = nf.load(args.load, False, ignoreDiag=_flag(args.ignoreDiag))
        _eval(nf, fm, task, args.test, args.predict, args.nFeatures, args.verbose)
        if args.dump:
            fm.dump(args.dump)
        return 0
    if args.solver == "hazan":
        return _train_hazan(nf, args, task)
    if args.solver == "gcd":
        raise ValueError("Solver gcd (greedy coordinate descent for convex factorization machines) is not supported by this "
                         "command line: the library runs it as nimfm_amd.newGreedyCD(...).fit(X, y, cfm) (refitFully = false); "
                         "use that, the reference's nimfm_cfm --solver gcd, or --solver hazan here")
    if args.solver not in ("sgd", "adagrad", "mbpsgd", "psgd", "pcd", "nmapgd", "fista", "katyusha"):
        if args.solver in ("cd", "als"):
            raise ValueError("Solver %s is not supported by this command line (sgd, adagrad, mbpsgd, pcd); coordinate descent "
                             "runs through nimfm_amd.newCD(...).fit(X, y, fm)" % args.solver)
        if args.solver == "pbcd":
            raise ValueError("Solver pbcd is not supported by this command line (sgd, adagrad, mbpsgd, pcd); proximal block "
                             "coordinate descent runs through nimfm_amd.newPBCD(...).fit(X, y, sfm)")
        raise ValueError("Solver %s is not supported on this path (sgd, adagrad, mbpsgd, pcd)" % args.solver)
    if args.solver == "pcd" and args.reg in ("l21", "squaredl21"):  # nimfm_sparsefm.nim:124-146
        raise ValueError("PCD cannot be used for %s." % ("L21" if args.reg == "l21" else "squaredL21"))
    if args.load:
        fm = nf.load(args.load, True)
    else:
        fm = nf.newFactorizationMachine(task, degree=args.degree, nComponents=args.nComponents, fitLower=args.fitLower,
                                        fitIntercept=_flag(args.fitIntercept), fitLinear=_flag(args.fitLinear),
                                        warmStart=False, randomState=args.randomState, scale=args.scale)
    X, y = nf.loadSVMLightFile(args.train, args.nFeatures)
    if args.verbose > 0:
        _echo_data_info(X)
    common = dict(maxIter=args.maxIter, eta0=args.eta0, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta,
                  loss=args.loss, verbose=args.verbose, tol=args.tol, shuffle=_flag(args.shuffle), mode=args.mode,
                  batch=args.batch, lossParam=args.threshold)
    if args.solver == "mbpsgd":
        regs = {"l1": nf.newL1, "l21": nf.newL21, "squaredl12": nf.newSquaredL12, "squaredl21": nf.newSquaredL21}
        if args.reg not in regs:
            raise ValueError("reg %s is not supported (l1, l21, squaredl12, squaredl21)" % args.reg)
        opt = nf.newMBPSGD(maxIter=args.maxIter, eta0=args.eta0, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta,
                           gamma=args.gamma, loss=args.loss, reg=regs[args.reg](), miniBatchSize=args.miniBatchSize,
                           scheduling=args.scheduling, power=args.power, verbose=args.verbose, tol=args.tol,
                           shuffle=_flag(args.shuffle), lossParam=args.threshold)
    elif args.solver == "psgd":  # built as trainInner builds mbpsgd (nimfm_sparsefm.nim:58-63), without the mini-batch size
        regs = {"l1": nf.newL1, "l21": nf.newL21, "squaredl12": nf.newSquaredL12, "squaredl21": nf.newSquaredL21,
                "omegati": nf.newOmegaTI, "omegacs": nf.newOmegaCS}
        if args.reg not in regs:
            raise ValueError("regularization %s is not supported" % args.reg)
        opt = nf.newPSGD(maxIter=args.maxIter, eta0=args.eta0, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta,
                         gamma=args.gamma, loss=args.loss, reg=regs[args.reg](), scheduling=args.scheduling, power=args.power,
                         verbose=args.verbose, tol=args.tol, shuffle=_flag(args.shuffle), lossParam=args.threshold)
    elif args.solver in ("nmapgd", "fista"):  # trainInner2 (nimfm_sparsefm.nim:47-57)
        regs = {"l1": nf.newL1, "l21": nf.newL21, "squaredl12": nf.newSquaredL12, "squaredl21": nf.newSquaredL21}
        if args.reg not in regs:
            raise ValueError("regularization %s is not supported" % args.reg)
        new = nf.newNMAPGD if args.solver == "nmapgd" else nf.newFISTA
        sigma = args.sigma if args.sigma is not None else (0.01 if args.solver == "nmapgd" else 1.0)
        opt = new(maxIter=args.maxIter, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta, gamma=args.gamma, loss=args.loss,
                  reg=regs[args.reg](), rho=args.rho, sigma=sigma, maxSearch=args.maxSearch, verbose=args.verbose, tol=args.tol,
                  lossParam=args.threshold)
    elif args.solver == "katyusha":  # trainInner2 (nimfm_sparsefm.nim:64-68): eta = --eta0; tau1 and tau2 keep newKatyusha's defaults
        regs = {"l1": nf.newL1, "l21": nf.newL21, "squaredl12": nf.newSquaredL12, "squaredl21": nf.newSquaredL21}
        if args.reg not in regs:
            raise ValueError("regularization %s is not supported" % args.reg)
        opt = nf.newKatyusha(maxIter=args.maxIter, eta=args.eta0, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta, gamma=args.gamma,
                             loss=args.loss, reg=regs[args.reg](), miniBatchSize=args.miniBatchSize, verbose=args.verbose, tol=args.tol,
                             shuffle=_flag(args.shuffle), lossParam=args.threshold)
    elif args.solver == "pcd":  # trainPCD (nimfm_sparsefm.nim:44-58): newSquaredL12() is column-wise
        regs = {"l1": nf.newL1, "squaredl12": nf.newSquaredL12}
        if args.reg not in regs:
            raise ValueError("reg %s is not supported for PCD (l1, squaredl12)" % args.reg)
        opt = nf.newPCD(maxIter=args.maxIter, alpha0=args.alpha0, alpha=args.alpha, beta=args.beta, gamma=args.gamma,
                        loss=args.loss, reg=regs[args.reg](), verbose=args.verbose, tol=args.tol, lossParam=args.threshold)
    elif args.solver == "sgd":
        cap = nf.suggestTouchCap(X, args.batch) if str(args.touchCap).lower() == "auto" else float(args.touchCap)
        opt = nf.newSGD(scheduling=args.scheduling, power=args.power, touchCap=cap, **common)
    else:
        opt = nf.newAdaGrad(adaCross=args.adaCross, **common)
    opt.fit(X, y, fm)
    if args.test:
        _eval(nf, fm, task, args.test, args.predict, args.nFeatures, args.verbose)
    if args.dump:
        fm.dump(args.dump)
    return 0


if __name__ == "__main__":
    sys.exit(main())
