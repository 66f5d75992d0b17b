"""nimfm_amd -- MI355X (gfx950) hot path for nimfm factorization machines.

Layout:
  csrc/      hand-written HIP kernels + the C ABI (include/nimfm_hip.h) -> lib/libnimfm_hip.so
  _capi.py   ctypes binding of that ABI (fails loudly when the library is missing)
  host.py    host-side mirror of the reference's Nim surface (newSGD(...).fit(X, y, fm), ...)
  dp.py      handles of the library's data-parallel groups (nfm_dp_*: RCCL between processes, peer sums inside one)
"""
from ._capi import NfmError, NotFittedError, build, lib  # noqa: F401
from .host import (ConvexFactorizationMachine, GreedyCD, newGreedyCD, Hazan, newConvexFactorizationMachine, newHazan, globalRand, FISTA, Katyusha, NMAPGD, PGD, newKatyusha, newFISTA, newNMAPGD, newPGD, L1, L21, MBPSGD, PSGD, newPSGD, OmegaCS, OmegaTI, PBCD, PCD, SquaredL12, SquaredL21, newL1, newL21, newMBPSGD, newOmegaCS, newOmegaTI, newPBCD, newPCD, predictAllWithGrad, newSquaredL12, newSquaredL21,  # noqa: F401
                   AdaGrad, CD, Context, CSRDataset, StreamCSRDataset, NimRand, randomNormal, randomize, FactorizationMachine, FieldAwareFactorizationMachine, SGD,  # noqa: F401
                   accuracy, convertSVMLightFile, default_context, expit, load, loadFFMFile, loadSVMLightFile, newAdaGrad, newCD, newCSRDataset, newCSRFieldDataset,
                   newFactorizationMachine, newFieldAwareFactorizationMachine, newSGD, newStreamCSRDataset, parseText, rmse, suggestTouchCap,
                   set_default_context, shuffle, vstack, hstack, normalize, loadUserItemRatingFile, parseUserItemRatingText,
                   dumpSVMLightFile, dumpFFMFile, formatText, formatF64, parseF64,
                   CSCDataset, newCSCDataset, toCSCDataset, toCSRDataset,
                   newStreamCSCDataset, transposeFile, convertFFMFile, dumpStreamFile, formatStream, loadStreamLabel)
