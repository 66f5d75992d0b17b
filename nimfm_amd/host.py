"""Host-side mirror of nimfm's FM surface over the C ABI (include/nimfm_hip.h).

Same names, argument meaning, defaults and error behaviour as the reference procs it stands in
for (citations relative to /root/reference/src/nimfm/), so that parity tests read like the
reference's own tests:

    newCSRDataset / newCSRFieldDataset       dataset.nim:116-123, tensor/sparse.nim:9-24
    newFactorizationMachine, init, decisionFunction, predict, predictProba, score
                                             model/factorization_machine.nim:43-139, model/fm_base.nim:13-48
    newFieldAwareFactorizationMachine        model/field_aware_factorization_machine.nim:24-92
    newSGD(...).fit(X, y, fm, callback)      optimizer/sgd.nim:23-52,261-328 (FFM: sgd_ffm.nim:49-106)
    newAdaGrad(...).fit(X, y, fm, callback)  optimizer/adagrad.nim:20-44,137-203 (FFM: adagrad_ffm.nim:11-66)
    fit(..., maxThreads=...)                 optimizer/sgd_multi.nim:40-42, adagrad_multi.nim:39-41

The epoch loop, shuffle, stopping criterion, verbose lines and callbacks run here exactly where
the Nim shim (nim/nimfm_hip.nim) runs them; everything per-sample runs in libnimfm_hip.so.
The reference is Nim and no Nim toolchain exists in the build image, so this Python module is the
executable stand-in for that shim (and what bench.py / torch.distributed drive).
"""
import ctypes as C
import mmap
import os
import math
from types import SimpleNamespace

import numpy as np

from . import _capi as capi


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


class Context:
    """One GPU + one HIP stream (one process per GPU)."""

    def __init__(self, device_id=0, stream=None):
        self.h = C.c_void_p()
        capi.check(capi.lib().nfm_ctx_create(device_id, stream, C.byref(self.h)))
        self.device_id = device_id

    def synchronize(self):
        capi.check(capi.lib().nfm_ctx_synchronize(self.h))

    def timing_enable(self, on=True):
        capi.check(capi.lib().nfm_ctx_timing_enable(self.h, int(on)))

    def timing_reset(self):
        capi.check(capi.lib().nfm_ctx_timing_reset(self.h))

    def timing_get(self, family):
        n, ms = C.c_int64(0), C.c_double(0.0)
        capi.check(capi.lib().nfm_ctx_timing_get(self.h, family.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def close(self):
        if self.h and capi.alive:
            capi.lib().nfm_ctx_destroy(self.h)
        self.h = C.c_void_p()


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def set_default_context(ctx):
    global _default_ctx
    _default_ctx = ctx


class CSRDataset:
    """dataset.nim:10-16 BaseDataset[CSRMatrix]; rows resident in HBM."""

    def __init__(self, data=None, indices=None, indptr=None, nSamples=0, nFeatures=0, fields=None, nFields=0,
                 ctx=None, _handle=None, _keep=None):
        self.ctx = ctx or default_context()
        self.nSamples, self._nFeatures, self.nFields = int(nSamples), int(nFeatures), int(nFields)
        self._keep = _keep
        if _handle is not None:
            self.h = _handle
            return
        data, indices, indptr = _f64(data), _i64(indices), _i64(indptr)
        if len(indptr) != self.nSamples + 1:
            raise ValueError("len(indptr) != nSamples + 1")
        if len(indices) != len(data) or (len(indptr) and indptr[-1] != len(data)):
            raise ValueError("indices/data/indptr sizes are inconsistent")
        fl = None if fields is None else _i64(fields)
        self.nnz = len(data)
        self.h = C.c_void_p()
        capi.check(capi.lib().nfm_dataset_create_csr(self.ctx.h, self.nSamples, self._nFeatures, _vp(indptr),
                                                     _vp(indices), _vp(data), _vp(fl), self.nFields, None,
                                                     C.byref(self.h)))

    @classmethod
    def from_device(cls, ctx, n, d, nnz, indptr_ptr, indices_ptr, data_ptr, y_ptr=None, fields_ptr=None, nFields=0,
                    keep=None):
        """Adopt device-resident arrays (raw device pointers, e.g. torch tensors' data_ptr())."""
        h = C.c_void_p()
        capi.check(capi.lib().nfm_dataset_create_csr_device(ctx.h, n, d, nnz, indptr_ptr, indices_ptr, data_ptr,
                                                            fields_ptr, nFields, y_ptr, C.byref(h)))
        ds = cls(nSamples=n, nFeatures=d, nFields=nFields, ctx=ctx, _handle=h, _keep=keep)
        ds.nnz = nnz
        return ds

    @classmethod
    def _from_loader(cls, ctx, h):
        """the object of a handle the library made: a CSRDataset or a CSCDataset, by the handle's layout"""
        n, d, nnz, nf, lay = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        capi.check(capi.lib().nfm_dataset_shape(h, C.byref(n), C.byref(d), C.byref(nnz), C.byref(nf)))
        capi.check(capi.lib().nfm_dataset_layout(h, C.byref(lay)))
        kind = CSCDataset if lay.value == capi.LAYOUT["csc"] else CSRDataset
        ds = kind(nSamples=n.value, nFeatures=d.value, nFields=nf.value, ctx=ctx, _handle=h)
        ds.nnz = nnz.value
        return ds

    def targets(self):
        """the targets stored with the dataset (the loaders' y)"""
        y = np.zeros(self.nSamples)
        capi.check(capi.lib().nfm_dataset_get_targets(self.h, _vp(y)))
        return y

    def rows_ascend(self):
        """True where every row stores its column ids in strictly ascending order (established when the dataset is made)"""
        a = C.c_int32()
        capi.check(capi.lib().nfm_dataset_rows_ascend(self.h, C.byref(a)))
        return bool(a.value)

    def to_host(self):
        """(indptr, indices, data, fields or None) in the reference's widths (tensor/sparse.nim:9-12, 19-24)"""
        indptr = np.zeros(self.nSamples + 1, dtype=np.int64)
        indices = np.zeros(self.nnz, dtype=np.int64)
        data = np.zeros(self.nnz)
        fields = np.zeros(self.nnz, dtype=np.int64) if self.nFields else None
        capi.check(capi.lib().nfm_dataset_get_csr(self.h, _vp(indptr), _vp(indices), _vp(data), _vp(fields)))
        return indptr, indices, data, fields

    def batch_plan(self, batch, begin=0, end=None, perm=None, device_order=None, n_aug=0, first_singleton=False,
                   want_tq=False, use_singles=False, sort_by_count=False):
        """The batch plan a mini-batch epoch over [begin, end) would run on, read back as a dict of integers and numpy
        arrays (nfm_dataset_plan_build / nfm_dataset_plan_get; diagnostic).  perm: a host order, indexed as the epoch
        indexes it; device_order = (seed, epoch): the order the device draws for that epoch of a shuffled fit."""
        L = capi.lib()
        end = self.nSamples if end is None else int(end)
        if perm is not None and device_order is not None:
            raise ValueError("perm and device_order exclude each other")
        order, seed, epoch, ph = capi.PLAN_ORDER["none"], 0, 0, None
        if perm is not None:
            ph = _i64(perm)
            if len(ph) < end:
                raise ValueError("perm is shorter than the range's end")
            order = capi.PLAN_ORDER["host"]
        elif device_order is not None:
            order, (seed, epoch) = capi.PLAN_ORDER["device"], device_order
        flags = sum(bit for name, bit in capi.PLAN_FLAGS.items()
                    if dict(first_singleton=first_singleton, want_tq=want_tq, use_singles=use_singles, sort_by_count=sort_by_count)[name])
        capi.check(L.nfm_dataset_plan_build(self.h, int(n_aug), order, _vp(ph), int(seed), int(epoch), int(begin), end, int(batch), flags))
        try:
            out = {}
            n, eb = C.c_int64(), C.c_int32()
            for name in capi.PLAN_SCALARS:
                v = np.zeros(1, dtype=np.int64)
                capi.check(L.nfm_dataset_plan_get(self.h, name.encode(), _vp(v), 8, C.byref(n), C.byref(eb)))
                out[name] = int(v[0])
            for name, dt in [(v, "<i8") for v in capi.PLAN_VECTORS] + list(capi.PLAN_ARRAYS.items()):
                capi.check(L.nfm_dataset_plan_get(self.h, name.encode(), None, 0, C.byref(n), C.byref(eb)))
                a = np.zeros(n.value, dtype=dt)
                if a.itemsize != eb.value:
                    raise capi.NfmError(capi.ERR_INVALID, "plan field %s has %d-byte elements" % (name, eb.value))
                if n.value:
                    capi.check(L.nfm_dataset_plan_get(self.h, name.encode(), _vp(a), a.nbytes, C.byref(n), C.byref(eb)))
                out[name] = a
            out["builder"] = capi.PLAN_BUILDER[out["builder"]]
            return out
        finally:
            capi.check(L.nfm_dataset_plan_release(self.h))

    def ingest_stats(self):
        """(bytes of text, upload ms, parse ms) of the loader that built this dataset"""
        b, u, p = C.c_int64(), C.c_double(), C.c_double()
        capi.check(capi.lib().nfm_dataset_ingest_stats(self.h, C.byref(b), C.byref(u), C.byref(p)))
        return b.value, u.value, p.value

    @property
    def nFeatures(self):
        return self._nFeatures

    @property
    def shape(self):
        return [self.nSamples, self._nFeatures]

    def set_targets(self, y):
        y = _f64(y)
        if len(y) != self.nSamples:
            raise ValueError("len(y) != nSamples")
        capi.check(capi.lib().nfm_dataset_set_targets(self.h, _vp(y)))

    def __getitem__(self, key):
        """X[indicesRow] / X[a..<b] (dataset.nim:319-369) as a new dataset made on the device: a list or integer array of
        row ids (repeats allowed), a slice or a range of step 1.  The ids are taken as the reference takes them: no
        wrap-around for negative ones (ValueError with checkIndicesRow's texts, dataset.nim:307-316)."""
        h = C.c_void_p()
        if isinstance(key, (slice, range)):
            if key.step not in (None, 1):
                raise ValueError("only slices of step 1 are supported")
            a = 0 if key.start is None else int(key.start)
            b = self.nSamples if key.stop is None else int(key.stop)
            capi.check(capi.lib().nfm_dataset_slice_rows(self.h, a, b, C.byref(h)))
        else:
            rows = np.asarray(key)
            if rows.ndim != 1 or (rows.size and rows.dtype.kind not in "iu"):
                raise TypeError("row ids must be a one-dimensional list or array of integers")
            rows = _i64(rows)
            capi.check(capi.lib().nfm_dataset_select_rows(self.h, _vp(rows), len(rows), C.byref(h)))
        return CSRDataset._from_loader(self.ctx, h)

    def _swap_handle(self, h):
        """the reference's in-place procs (normalize): the object takes the new dataset's handle and destroys the old one;
        arrays adopted by from_device are let go"""
        old, self.h = self.h, h
        self._keep = None
        n, d, nnz, nf = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        capi.check(capi.lib().nfm_dataset_shape(h, C.byref(n), C.byref(d), C.byref(nnz), C.byref(nf)))
        self.nSamples, self._nFeatures, self.nnz, self.nFields = n.value, d.value, nnz.value, nf.value
        capi.check(capi.lib().nfm_dataset_destroy(old))

    def __del__(self):
        try:
            if capi.alive and getattr(self, "h", None):
                capi.lib().nfm_dataset_destroy(self.h)
                self.h = None
        except Exception:
            pass


class CSCDataset(CSRDataset):
    """dataset.nim:18-22 BaseDataset[CSCMatrix]: columns resident in HBM -- indptr [nFeatures + 1], indices (sample ids) and
    data [nnz] -- beside the row twin the library makes of them, which decisionFunction, score and the
    column-wise solvers (newCD, newPCD, newPBCD, newHazan, newGreedyCD) run on.  The row-wise solvers, X[indices], shuffle
    and the text dumps refuse it (ValueError naming toCSRDataset), as the reference does at compile time."""

    def __init__(self, data=None, indices=None, indptr=None, nSamples=0, nFeatures=0, fields=None, nFields=0,
                 ctx=None, _handle=None, _keep=None):
        if _handle is not None:
            super().__init__(nSamples=nSamples, nFeatures=nFeatures, ctx=ctx, _handle=_handle, _keep=_keep)
            return
        if fields is not None or nFields:
            raise ValueError("there is no field-aware CSCDataset")
        self.ctx = ctx or default_context()
        self.nSamples, self._nFeatures, self.nFields = int(nSamples), int(nFeatures), 0
        self._keep = None
        data, indices, indptr = _f64(data), _i64(indices), _i64(indptr)
        if len(indptr) != self._nFeatures + 1:
            raise ValueError("len(indptr) != nFeatures + 1")
        if len(indices) != len(data) or (len(indptr) and indptr[-1] != len(data)):
            raise ValueError("indices/data/indptr sizes are inconsistent")
        self.nnz = len(data)
        self.h = C.c_void_p()
        capi.check(capi.lib().nfm_dataset_create_csc(self.ctx.h, self.nSamples, self._nFeatures, _vp(indptr), _vp(indices),
                                                     _vp(data), None, C.byref(self.h)))

    @classmethod
    def from_device(cls, ctx, n, d, nnz, indptr_ptr, indices_ptr, data_ptr, y_ptr=None):
        """A CSCDataset of device-resident COLUMN arrays (raw device pointers: indptr int64[d + 1], indices int32[nnz] sample
        ids, data float64[nnz]; y float64[n] or None).  The arrays are read once: the dataset owns copies (and its row twin),
        so the caller need not keep them alive (CSRDataset.from_device adopts its arrays instead)."""
        h = C.c_void_p()
        capi.check(capi.lib().nfm_dataset_create_csc_device(ctx.h, n, d, nnz, indptr_ptr, indices_ptr, data_ptr, y_ptr, C.byref(h)))
        return CSRDataset._from_loader(ctx, h)

    def to_host(self):
        """(indptr, indices, data) of the columns in the reference's widths (CSCMatrix, tensor/sparse.nim:14-17)"""
        indptr = np.zeros(self._nFeatures + 1, dtype=np.int64)
        indices = np.zeros(self.nnz, dtype=np.int64)
        data = np.zeros(self.nnz)
        capi.check(capi.lib().nfm_dataset_get_csc(self.h, _vp(indptr), _vp(indices), _vp(data)))
        return indptr, indices, data

    def __getitem__(self, key):
        """X[a..<b] (tensor/sparse.nim:300-330): per column the entries of samples a .. b - 1, ids rebased; a slice or a
        range of step 1.  X[indices] is refused as the reference refuses it (:298)."""
        if not isinstance(key, (slice, range)):
            raise ValueError("Accessing row vectors by openarray is not supported for CSCMatrix: slice it (X[a:b]) or convert "
                             "it with toCSRDataset")
        return super().__getitem__(key)


def _row_major(X, what):
    """what takes rows in storage order refuses a CSCDataset (the reference: at compile time)"""
    if isinstance(X, CSCDataset):
        raise ValueError("%s takes a row-major dataset, not a CSCDataset: convert it with toCSRDataset" % what)
    return X


def newCSCDataset(data, indices, indptr, nSamples, nFeatures, ctx=None):
    """dataset.nim:124-129"""
    return CSCDataset(data, indices, indptr, nSamples, nFeatures, ctx=ctx)


def toCSCDataset(X):
    """tensor/sparse.nim:510-527 on the device: column j lists its entries by ascending sample id, entries of one sample
    that repeat j in the row's storage order; the targets are carried over.  A new dataset; X is only read."""
    _resident(X, "toCSCDataset")
    if X.nFields:
        raise ValueError("toCSCDataset of a field-aware dataset: there is no CSCFieldDataset on the device")
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_to_csc(X.h, C.byref(h)))
    return CSRDataset._from_loader(X.ctx, h)


def toCSRDataset(X):
    """tensor/sparse.nim:490-507 on the device: row i lists its entries by ascending column id, repeats in column-storage
    order; the targets are carried over.  A new dataset; X is only read."""
    _resident(X, "toCSRDataset")
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_to_csr(X.h, C.byref(h)))
    return CSRDataset._from_loader(X.ctx, h)


def _as_layout(ds, layout):
    """a loader's row-major result in the layout asked for"""
    if layout not in capi.LAYOUT:
        raise ValueError("layout must be one of %s" % sorted(capi.LAYOUT))
    return toCSCDataset(ds) if layout == "csc" else ds


def newCSRDataset(data, indices, indptr, nSamples, nFeatures, ctx=None):
    return CSRDataset(data, indices, indptr, nSamples, nFeatures, ctx=ctx)


def newCSRFieldDataset(data, indices, indptr, fields, nSamples, nFeatures, nFields, ctx=None):
    return CSRDataset(data, indices, indptr, nSamples, nFeatures, fields=fields, nFields=nFields, ctx=ctx)


# ------------------------------------------------------------------------------------------------
# Nim's global random number generator, as the reference uses it: randomize(seed) in init
# (model/factorization_machine.nim:131), randomNormal for P (tensor/tensor.nim:561-580), shuffle(indices) in fit
# (optimizer/sgd.nim:297).  The procedures live in the library (nfm_rng_*, host code); the generator itself is
# outside the reference tree and restated from memory (unverified, include/nimfm_hip.h).
# ------------------------------------------------------------------------------------------------
class NimRand:
    def __init__(self, seed=None):
        self.state = (C.c_uint64 * 2)(0x69B4C98CB8530805, 0xFED1DD3004688D68)  # Nim's default global state
        if seed is not None:
            self.randomize(seed)

    def randomize(self, seed):
        capi.check(capi.lib().nfm_rng_randomize(int(seed), self.state))

    def randomNormal(self, shape, loc=0.0, scale=1.0):
        """tensor/tensor.nim:561-580: row-major fill, the cosine / sine halves of one draw on consecutive elements"""
        out = np.empty(int(np.prod(shape)), dtype=np.float64)
        capi.check(capi.lib().nfm_rng_random_normal(self.state, out.size, float(loc), float(scale), _vp(out)))
        return out.reshape(shape)

    def rand(self, n, max=1.0):
        """n draws of rand(max) (Nim's rand(max: float)) in sequence, e.g. the `2*rand(1.0) - 1.0` of powerMethod's start
        vector (tensor/tensor.nim:920-921)"""
        out = np.empty(int(n), dtype=np.float64)
        capi.check(capi.lib().nfm_rng_rand_uniform(self.state, out.size, float(max), _vp(out)))
        return out

    def shuffle(self, x):
        """in place, Nim's shuffle: for i in countdown(high, 1): swap(x[i], x[rand(i)])"""
        assert x.dtype == np.int64 and x.flags["C_CONTIGUOUS"]
        capi.check(capi.lib().nfm_rng_shuffle(self.state, _vp(x), len(x)))

    def shuffleForward(self, x):
        """in place, the draw of shuffle(X, y) (dataset.nim:388-394): for i ascending, j = rand(n-1-i), swap(x[i], x[i+j])"""
        assert x.dtype == np.int64 and x.flags["C_CONTIGUOUS"]
        capi.check(capi.lib().nfm_rng_shuffle_forward(self.state, _vp(x), len(x)))


_global_rng = None


def globalRand():
    global _global_rng
    if _global_rng is None:
        _global_rng = NimRand()
    return _global_rng


def randomize(seed):
    globalRand().randomize(seed)


def randomNormal(shape, loc=0.0, scale=1.0, uniform=None):
    """tensor/tensor.nim:561-580.  uniform: an explicit stream of rand(1.0) draws (array, 2 per pair of elements)
    instead of the global generator -- the same pairing and fill order, vectorised."""
    if uniform is None:
        return globalRand().randomNormal(shape, loc, scale)
    n = int(np.prod(shape))
    u = _f64(uniform)[: 2 * ((n + 1) // 2)]
    if len(u) < 2 * ((n + 1) // 2):
        raise ValueError("randomNormal needs %d uniform draws" % (2 * ((n + 1) // 2)))
    x, y = u[0::2], u[1::2]
    r = np.sqrt(-2 * np.log(1.0 - x))
    z = np.empty(2 * len(x))
    z[0::2] = r * np.cos(2 * math.pi * y)
    z[1::2] = r * np.sin(2 * math.pi * y)
    return (loc + z[:n] * scale).reshape(shape)


def expit(x):
    """utils.nim:33"""
    x = np.asarray(x, dtype=np.float64)
    return np.exp(np.minimum(0.0, x)) / (1.0 + np.exp(-np.abs(x)))


def rmse(yTrue, yScore):
    """metrics.nim:5-13"""
    yTrue, yScore = _f64(yTrue), _f64(yScore)
    if len(yTrue) != len(yScore):
        raise ValueError("len(yScore)=%d, but len(yTrue)=%d" % (len(yScore), len(yTrue)))
    return math.sqrt(float(np.sum((yScore - yTrue) ** 2)) / len(yTrue))


def accuracy(yTrue, yPred):
    """metrics.nim:39-47"""
    yTrue, yPred = np.asarray(yTrue), np.asarray(yPred)
    if len(yTrue) != len(yPred):
        raise ValueError("len(yPred)=%d, but len(yTrue)=%d" % (len(yPred), len(yTrue)))
    return float(np.mean(yTrue == yPred))


class _ModelBase:
    """Fields/procs shared by FM and FFM (model/fm_base.nim)."""

    def __init__(self):
        self._h = None
        self._gen = 0  # bumps whenever the device model is released: optimizers built on it are stale then
        self._ctx = None
        self._dirty = True
        self._P = None
        self._w = None
        self._intercept = 0.0
        self.isInitialized = False

    # host copies are the public truth (fm.P / fm.w / fm.intercept); assigning marks the device copy stale
    @property
    def P(self):
        return self._P

    @P.setter
    def P(self, v):
        self._P = _f64(v)
        self._dirty = True

    @property
    def w(self):
        return self._w

    @w.setter
    def w(self, v):
        self._w = _f64(v)
        self._dirty = True

    @property
    def intercept(self):
        return self._intercept

    @intercept.setter
    def intercept(self, v):
        self._intercept = float(v)
        self._dirty = True

    def checkInitialized(self):
        if not self.isInitialized:
            raise capi.NotFittedError(capi.ERR_NOT_FITTED, "Factorization machines is not fitted.")

    def _handle(self, ctx):
        if self._h is None or self._ctx is not ctx:
            self._release()
            cfg = self._cfg()
            self._h = C.c_void_p()
            capi.check(capi.lib().nfm_model_create(ctx.h, C.byref(cfg), C.byref(self._h)))
            self._ctx = ctx
            self._dirty = True
        return self._h

    def _push(self, ctx):
        h = self._handle(ctx)
        if self._dirty:
            lams = getattr(self, "lams", None)
            capi.check(capi.lib().nfm_model_set_params(h, _vp(self._P), _vp(self._w), self._intercept,
                                                       None if lams is None else _vp(_f64(lams))))
            self._dirty = False
        return h

    def _pull(self):
        b = C.c_double(0.0)
        capi.check(capi.lib().nfm_model_get_params(self._h, _vp(self._P), _vp(self._w), C.byref(b)))
        self._intercept = b.value
        self._dirty = False

    def _release(self):
        if self._h is not None:
            self._gen += 1
            if capi.alive:
                capi.lib().nfm_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def decisionFunction(self, X):
        """model/factorization_machine.nim:100-122 / field_aware_factorization_machine.nim:52-76"""
        self.checkInitialized()
        self._check_shapes(X)
        if isinstance(X, StreamCSRDataset):  # block by block
            return np.concatenate([self.decisionFunction(X.load(r0, r1)) for r0, r1 in X.blocks()] or [np.zeros(0)])
        h = self._push(X.ctx)
        out = np.empty(X.nSamples, dtype=np.float64)
        capi.check(capi.lib().nfm_decision_function(h, X.h, _vp(out)))
        return out

    def predict(self, X):
        """model/fm_base.nim:18-20"""
        return np.sign(self.decisionFunction(X)).astype(np.int64)

    def predictProba(self, X):
        """model/fm_base.nim:23-26"""
        return expit(self.decisionFunction(X))

    def checkTarget(self, y):
        """model/fm_base.nim:29-36"""
        y = _f64(y)
        return np.sign(y) if self.task == "classification" else y

    def score(self, X, y):
        """model/fm_base.nim:39-48: rmse (regression) or accuracy of the signs (classification) of
        decisionFunction(X) against y -- reduced on the device, only the scalar comes back."""
        self.checkInitialized()
        self._check_shapes(X)
        X.set_targets(_f64(y))
        out = C.c_double()
        capi.check(capi.lib().nfm_score(self._push(X.ctx), X.h, C.byref(out)))
        return out.value

    def metrics(self, X, y):
        """rmse, accuracy (of signs) and rocauc (pos = 1) of decisionFunction(X) against y
        (metrics.nim:5-13, 39-47, 76-103), computed on the device."""
        self.checkInitialized()
        self._check_shapes(X)
        X.set_targets(_f64(y))
        r, a, u = C.c_double(), C.c_double(), C.c_double()
        capi.check(capi.lib().nfm_metrics(self._push(X.ctx), X.h, C.byref(r), C.byref(a), C.byref(u)))
        return {"rmse": r.value, "accuracy": a.value, "rocauc": u.value}


def _task_name(task):
    t = {"r": "regression", "c": "classification"}.get(task, task)
    if t not in ("regression", "classification"):
        raise ValueError("unknown task %r" % (task,))
    return t


class FactorizationMachine(_ModelBase):
    def __init__(self, task, degree=2, nComponents=30, fitLower="explicit", fitIntercept=True, fitLinear=True,
                 warmStart=False, randomState=1, scale=0.01):
        super().__init__()
        self.task = _task_name(task)
        if degree < 1:
            raise ValueError("degree < 1.")
        if nComponents < 1:
            raise ValueError("nComponents < 1.")
        if fitLower not in capi.LOWER:
            raise ValueError("unknown fitLower %r" % (fitLower,))
        self.degree, self.nComponents, self.fitLower = int(degree), int(nComponents), fitLower
        self.fitIntercept, self.fitLinear, self.warmStart = bool(fitIntercept), bool(fitLinear), bool(warmStart)
        self.randomState, self.scale = int(randomState), float(scale)
        self.lams = np.ones(self.nComponents)
        self._d = None

    @property
    def nAugments(self):
        """model/factorization_machine.nim:81-86"""
        if self.fitLower == "augment":
            return self.degree - 2 if self.fitLinear else self.degree - 1
        return 0

    @property
    def nOrders(self):
        """model/factorization_machine.nim:89-97"""
        if self.degree == 1:
            return 0
        return self.degree - 1 if self.fitLower == "explicit" else 1

    def _cfg(self):
        return capi.ModelCfg(capi.KIND_FM, capi.TASK[self.task], self.degree, self.nComponents,
                             capi.LOWER[self.fitLower], int(self.fitIntercept), int(self.fitLinear), 0,
                             int(self._d), 0)

    def _check_shapes(self, X):
        if X.nFeatures + self.nAugments != self._P.shape[2]:
            raise ValueError("Invalid nFeatures.")

    def init(self, X, force=False):
        """model/factorization_machine.nim:125-139: randomize(randomState); w = 0; P = randomNormal([nOrders,
        nComponents, nFeatures + nAugments], scale) -- Box-Muller pairs along the row-major fill -- intercept = 0.
        (The generator behind randomize / rand is Nim's stdlib, restated unverified: see NimRand.)"""
        if force or not (self.warmStart and self.isInitialized):
            d = X.nFeatures
            randomize(self.randomState)
            if self._d != d:
                self._release()
            self._d = d
            self.w = np.zeros(d)
            self.P = randomNormal((self.nOrders, self.nComponents, d + self.nAugments), scale=self.scale)
            self.intercept = 0.0
        self.isInitialized = True

    def _cross_args(self, U, V, what):
        self.checkInitialized()
        for X in (U, V):
            if not isinstance(X, CSRDataset):  # a dataset used in row blocks has no resident handle
                raise capi.NfmError(capi.ERR_UNSUPPORTED, "%s needs datasets resident on the device, not %s: materialise the pairs, "
                                    "hstack(U[rep], V[tile]), block by block and call decisionFunction" % (what, type(X).__name__))
        return self._push(U.ctx)

    def crossDecisionFunction(self, U, V):
        """-> float64 [nU, nV]: [i][j] is decisionFunction (model/factorization_machine.nim:100-122, kernels.nim:59-64) of row
        i of U followed by row j of V, i.e. of row i * nV + j of hstack(U[rep], V[tile]) (tensor/sparse.nim:671-698), which is
        never made.  A FactorizationMachine of degree 2; everything else is refused by the library."""
        h = self._cross_args(U, V, "crossDecisionFunction")
        out = np.empty((U.nSamples, V.nSamples), dtype=np.float64)
        capi.check(capi.lib().nfm_cross_decision_function(h, U.h, V.h, _vp(out)))
        return out

    def recommend(self, U, V, topK, chunkItems=0):
        """-> (ids int64 [nU, topK], scores float64 [nU, topK]): per row of U the topK rows of V by descending
        crossDecisionFunction, then ascending id (NaN below every number) -- the same bits, ranked on the device without the
        nU x nV scores being stored.  1 <= topK <= min(nV, 256).  chunkItems: the items one workgroup ranks (0: the
        library's choice); the result does not depend on it."""
        h = self._cross_args(U, V, "recommend")
        K = int(topK)
        Ka = K if 1 <= K <= 256 else 0  # (out of range: the library refuses before it writes)
        ids = np.empty((U.nSamples, Ka), dtype=np.int64)
        scores = np.empty((U.nSamples, Ka), dtype=np.float64)
        capi.check(capi.lib().nfm_cross_topk(h, U.h, V.h, K, int(chunkItems), _vp(ids), _vp(scores)))
        return ids, scores

    def set_params(self, P, w, intercept):
        """Inject parameters (the reference's warm-start path: init is skipped when
        warmStart and isInitialized, factorization_machine.nim:129)."""
        P = _f64(P)
        if P.ndim != 3 or P.shape[0] != self.nOrders or P.shape[1] != self.nComponents:
            raise ValueError("P must have shape [nOrders, nComponents, nFeatures+nAugments]")
        d = P.shape[2] - self.nAugments
        if self._d != d:
            self._release()
        self._d = d
        self.P, self.w, self.intercept = P.copy(), _f64(w).copy(), intercept
        if len(self._w) != d:
            raise ValueError("len(w) != nFeatures")
        self.isInitialized = True


def _nim_float(v):
    """Nim's `$float64`: the shortest form that reads back exactly (repr), "inf"/"nan" spelled Nim's way"""
    v = float(v)
    if v != v:
        return "nan"
    if v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    return repr(v)


def _number_lines_py(rows):
    """the number block of a model dump, one line per row: the values separated by one space, "\\n" after each row"""
    return "".join(" ".join(_nim_float(v) for v in r) + "\n" for r in rows)


_DUMP_DEVICE_MIN = 65536  # a block of at least this many values is formatted on the device (nfm_format_f64)


def _have_device():
    n = C.c_int32(0)
    return capi.lib().nfm_device_count(C.byref(n)) == capi.NFM_OK and n.value > 0


def formatF64(values, ctx=None):
    """a 2-D block of float64 -> the bytes of its lines (nfm_format_f64: formatted on the device)"""
    a = np.ascontiguousarray(values, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("formatF64 needs a 2-D block")
    ctx = ctx or default_context()
    n = C.c_int64(0)
    capi.check(capi.lib().nfm_format_f64(ctx.h, _vp(a), a.shape[0], a.shape[1], None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    capi.check(capi.lib().nfm_format_f64(ctx.h, _vp(a), a.shape[0], a.shape[1], buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def _number_lines(rows):
    a = np.asarray(rows, dtype=np.float64)
    if a.ndim == 2 and a.size >= _DUMP_DEVICE_MIN and _have_device():
        return formatF64(a).decode("ascii")
    return _number_lines_py(rows)


_LOAD_DEVICE_MIN = 32768  # a block of at least this many values is parsed on the device (nfm_parse_f64); from the sweep of
# tools/model_load_time.py


def parseF64(text, nRows, rowLen, ctx=None, chunkBytes=0, out=None):
    """the first nRows lines of `text` (bytes, or any buffer such as an mmap or a memoryview of one: not copied), rowLen
    numbers each -> (float64 array [nRows, rowLen], bytes consumed), parsed on the device (nfm_parse_f64).  None: the text
    is not clean -- a token that is not a number to its last byte, a short line, too few lines -- and the caller reads it
    with its own parser.  out: a C-contiguous float64 array [nRows, rowLen] to fill (unspecified when None comes back)."""
    raw = np.frombuffer(text, dtype=np.uint8)
    if out is None:
        out = np.empty((int(nRows), int(rowLen)))
    elif out.shape != (nRows, rowLen) or out.dtype != np.float64 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("parseF64: out must be a writable C-contiguous float64 array [nRows, rowLen]")
    ctx = ctx or default_context()
    consumed, clean = C.c_int64(0), C.c_int32(0)
    capi.check(capi.lib().nfm_parse_f64(ctx.h, raw.ctypes.data if raw.size else None, raw.size, int(nRows), int(rowLen),
                                        int(chunkBytes), _vp(out), C.byref(consumed), C.byref(clean)))
    return (out, consumed.value) if clean.value else None


class _DumpText:
    """A model dump read through a read-only mapping, line by line as `open(fname).read().split("\\n")` hands them out
    (universal newlines: "\\r\\n" and a lone "\\r" end a line too; after the last line StopIteration), without holding
    the text as Python objects.  block() reads the number lines of a "lams:" / "P[o]:" / "w:" block."""

    def __init__(self, fname):
        with open(os.path.expanduser(fname), "rb") as f:
            self.buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(f.fileno()).st_size else b""
        self.pos = 0
        self.pending = []   # lines a lone "\r" cut off the raw line last read
        self.done = False

    def __iter__(self):
        return self

    def __next__(self):
        if self.pending:
            return self.pending.pop(0)
        if self.done:
            raise StopIteration
        e = self.buf.find(b"\n", self.pos)
        if e < 0:
            raw, self.pos, self.done = self.buf[self.pos:], len(self.buf), True
        else:
            raw, self.pos = self.buf[self.pos:e], e + 1
        if e >= 0 and raw.endswith(b"\r"):
            raw = raw[:-1]
        parts = raw.decode().split("\r")
        self.pending = parts[1:]
        return parts[0]

    def peek(self, n):
        """the first n lines, without moving"""
        saved = self.pos, list(self.pending), self.done
        out = []
        for line in self:
            out.append(line)
            if len(out) == n:
                break
        self.pos, self.pending, self.done = saved[0], saved[1], saved[2]
        return out

    def block(self, n_rows, row_len, out=None):
        """the next n_rows lines as a float64 array [n_rows, row_len] (out, when given) parsed on the device, the reader moved
        past them; None (and nothing moved) for a small block, without a device, or when the text is not clean: the caller
        then reads the lines one by one"""
        if self.pending or self.done or n_rows < 1 or row_len < 1 or n_rows * row_len < _LOAD_DEVICE_MIN or not _have_device():
            return None
        got = parseF64(memoryview(self.buf)[self.pos:], n_rows, row_len, out=out)
        if got is None:
            return None
        start = -(-self.pos // mmap.PAGESIZE) * mmap.PAGESIZE
        self.pos += got[1]
        stop = self.pos // mmap.PAGESIZE * mmap.PAGESIZE
        if stop > start and isinstance(self.buf, mmap.mmap):  # the block's pages are not read again: hand them back
            self.buf.madvise(mmap.MADV_DONTNEED, start, stop - start)
        self.done = self.pos >= len(self.buf) and self.buf[self.pos - 1:self.pos] != b"\n"
        return got[0]


def _floats(line):
    return [float(v) for v in line.split(" ") if v]


def _dump_fm(self, fname):
    """model/factorization_machine.nim:142-165: the reference's text model format"""
    self.checkInitialized()
    P, w = self.P, self.w
    d = P.shape[2] - self.nAugments
    with open(os.path.expanduser(fname), "w") as f:
        f.write("task: %s\n" % self.task)
        f.write("nFeatures: %d\n" % d)
        f.write("degree: %d\n" % self.degree)
        f.write("nComponents: %d\n" % self.nComponents)
        f.write("fitLower: %s\n" % self.fitLower)
        f.write("fitIntercept: %s\n" % ("true" if self.fitIntercept else "false"))
        f.write("fitLinear: %s\n" % ("true" if self.fitLinear else "false"))
        f.write("randomState: %d\n" % self.randomState)
        f.write("scale: %s\n" % _nim_float(self.scale))
        f.write("lams:\n")
        f.write(_number_lines([self.lams]))
        for order in range(P.shape[0]):
            f.write("P[%d]:\n" % order)
            f.write(_number_lines(P[order, :self.nComponents]))
        f.write("w:\n")
        f.write(_number_lines([w]))
        f.write("intercept: %s\n" % _nim_float(self.intercept))


FactorizationMachine.dump = _dump_fm


def load(fname, warmStart, ignoreDiag=True):
    """model/factorization_machine.nim:168-220 `load(fm, fname, warmStart)`: -> FactorizationMachine.  A dump of a
    ConvexFactorizationMachine (its fifth line is `maxComponents:`) is read by convex_factorization_machine.nim:111-164
    instead; that format does not store ignoreDiag, so the caller gives it."""
    it = _DumpText(fname)
    lines = it.peek(5)
    if len(lines) > 4 and lines[4].startswith("maxComponents:"):
        return _load_cfm(it, warmStart, ignoreDiag)
    if len(lines) > 1 and lines[1].startswith("nFields:"):  # a FieldAwareFactorizationMachine's dump
        return _load_ffm(it, warmStart)

    def field():
        return next(it).split(" ")[1]

    task = field()
    d = int(field())
    degree = int(field())
    k = int(field())
    fit_lower = field()
    fit_intercept = field().lower() in ("true", "y", "yes", "1", "on")  # Nim's parseBool
    fit_linear = field().lower() in ("true", "y", "yes", "1", "on")
    random_state = int(field())
    scale = float(field())
    fm = FactorizationMachine(task, degree, k, fit_lower, fit_intercept, fit_linear, bool(warmStart), random_state, scale)
    next(it)  # "lams:"
    lams = it.block(1, k)
    lams = lams[0] if lams is not None else np.array(_floats(next(it))[:k])
    P = np.zeros((fm.nOrders, k, d + fm.nAugments))
    for order in range(fm.nOrders):
        next(it)  # "P[order]:"
        if it.block(k, d + fm.nAugments, out=P[order]) is not None:
            continue
        for s_ in range(k):
            P[order, s_] = _floats(next(it))[: d + fm.nAugments]
    next(it)  # "w:"
    w = it.block(1, d)
    w = w[0] if w is not None else np.array(_floats(next(it))[:d])
    if len(w) != d:
        w = np.zeros(d)
    intercept = float(next(it).split(" ")[1])
    fm.set_params(P, w, intercept)
    fm.lams = lams
    return fm


class FieldAwareFactorizationMachine(_ModelBase):
    def __init__(self, task, nComponents=10, fitIntercept=True, fitLinear=True, warmStart=False, randomState=1,
                 scale=0.01):
        super().__init__()
        self.task = _task_name(task)
        if nComponents < 1:
            raise ValueError("nComponents < 1.")
        self.nComponents = int(nComponents)
        self.fitIntercept, self.fitLinear, self.warmStart = bool(fitIntercept), bool(fitLinear), bool(warmStart)
        self.randomState, self.scale = int(randomState), float(scale)
        self._d = None
        self._F = None

    nAugments = 0  # model/field_aware_factorization_machine.nim:49

    def _cfg(self):
        return capi.ModelCfg(capi.KIND_FFM, capi.TASK[self.task], 2, self.nComponents, 0, int(self.fitIntercept),
                             int(self.fitLinear), 0, int(self._d), int(self._F))

    def _check_shapes(self, X):
        if X.nFeatures != self._P.shape[1]:
            raise ValueError("Invalid nFeatures.")
        if X.nFields != self._P.shape[0]:
            raise ValueError("Invalid nFields.")

    def init(self, X, force=False):
        """model/field_aware_factorization_machine.nim:79-92"""
        if force or not (self.warmStart and self.isInitialized):
            d, F = X.nFeatures, X.nFields
            randomize(self.randomState)
            if (self._d, self._F) != (d, F):
                self._release()
            self._d, self._F = d, F
            self.w = np.zeros(d)
            self.P = randomNormal((F, d, self.nComponents), scale=self.scale)
            self.intercept = 0.0
        self.isInitialized = True

    def set_params(self, P, w, intercept):
        P = _f64(P)
        if P.ndim != 3 or P.shape[2] != self.nComponents:
            raise ValueError("P must have shape [nFields, nFeatures, nComponents]")
        if (self._d, self._F) != (P.shape[1], P.shape[0]):
            self._release()
        self._F, self._d = P.shape[0], P.shape[1]
        self.P, self.w, self.intercept = P.copy(), _f64(w).copy(), intercept
        self.isInitialized = True


def _dump_ffm(self, fname):
    """model/field_aware_factorization_machine.nim:95-116: the reference's text model format"""
    self.checkInitialized()
    P, w = self.P, self.w
    with open(os.path.expanduser(fname), "w") as f:
        f.write("task: %s\n" % self.task)
        f.write("nFields: %d\n" % P.shape[0])
        f.write("nFeatures: %d\n" % P.shape[1])
        f.write("nComponents: %d\n" % self.nComponents)
        f.write("fitIntercept: %s\n" % ("true" if self.fitIntercept else "false"))
        f.write("fitLinear: %s\n" % ("true" if self.fitLinear else "false"))
        f.write("randomState: %d\n" % self.randomState)
        f.write("scale: %s\n" % _nim_float(self.scale))
        for fld in range(P.shape[0]):
            f.write("P[%d]:\n" % fld)
            f.write(_number_lines(P[fld]))
        f.write("w:\n")
        f.write(_number_lines([w]))
        f.write("intercept: %s\n" % _nim_float(self.intercept))


FieldAwareFactorizationMachine.dump = _dump_ffm


def _load_ffm(it, warmStart):
    """model/field_aware_factorization_machine.nim:119-158; it: the dump's lines (_DumpText)"""

    def field():
        return next(it).split(" ")[1]

    def truth(v):
        return v.lower() in ("true", "y", "yes", "1", "on")  # Nim's parseBool

    task = field()
    F, d, k = int(field()), int(field()), int(field())
    fit_intercept, fit_linear = truth(field()), truth(field())
    random_state, scale = int(field()), float(field())
    ffm = FieldAwareFactorizationMachine(task, k, fit_intercept, fit_linear, bool(warmStart), random_state, scale)
    P = np.zeros((F, d, k))
    for fld in range(F):
        next(it)  # "P[field]:"
        if it.block(d, k, out=P[fld]) is not None:
            continue
        for j in range(d):
            P[fld, j] = _floats(next(it))[:k]
    next(it)  # "w:"
    w = it.block(1, d)
    w = w[0] if w is not None else np.array(_floats(next(it))[:d])
    intercept = float(next(it).split(" ")[1])
    ffm.set_params(P, w, intercept)
    return ffm


class ConvexFactorizationMachine(_ModelBase):
    """model/convex_factorization_machine.nim:6-60: P [nComponents][nFeatures], lams [nComponents], w, intercept; nComponents
    grows from 0 to maxComponents while newHazan(...).fit or newGreedyCD(...).fit adds basis vectors.  decisionFunction / predict / predictProba / score
    / metrics are _ModelBase's, on a device handle of the convex kind (nfm_cfm_create): with ignoreDiag the ANOVA kernel of
    degree 2, else the polynomial kernel (kernels.nim:22-43,67-79)."""
    degree = 2
    nAugments = 0

    def __init__(self, task, maxComponents=30, fitIntercept=True, fitLinear=True, ignoreDiag=True, warmStart=False):
        super().__init__()
        self.task = _task_name(task)
        if maxComponents < 1:
            raise ValueError("maxComponents < 1.")
        self.maxComponents = int(maxComponents)
        self.fitIntercept, self.fitLinear = bool(fitIntercept), bool(fitLinear)
        self.ignoreDiag, self.warmStart = bool(ignoreDiag), bool(warmStart)
        self._lams = np.zeros(0)
        self._d = None

    @property
    def lams(self):
        return self._lams

    @lams.setter
    def lams(self, v):
        self._lams = _f64(v)
        self._dirty = True

    @property
    def nComponents(self):
        return len(self._lams)

    def _check_shapes(self, X):
        if X.nFeatures != self._P.shape[1]:
            raise ValueError("Invalid nFeatures.")

    def _handle(self, ctx):
        if self._h is None or self._ctx is not ctx:
            self._release()
            self._h = C.c_void_p()
            capi.check(capi.lib().nfm_cfm_create(ctx.h, capi.TASK[self.task], self.maxComponents, int(self.fitIntercept),
                                                 int(self.fitLinear), int(self.ignoreDiag), int(self._d), C.byref(self._h)))
            self._ctx = ctx
            self._dirty = True
        return self._h

    def _push(self, ctx):
        h = self._handle(ctx)
        if self._dirty:
            nc = self.nComponents
            if self._P.shape != (nc, self._d) or nc > self.maxComponents:
                raise ValueError("P must have shape [len(lams), nFeatures] with len(lams) <= maxComponents")
            capi.check(capi.lib().nfm_cfm_set_params(h, nc, _vp(self._P), _vp(self._lams), _vp(self._w), self._intercept))
            self._dirty = False
        return h

    def _pull(self):
        nc, b = C.c_int32(0), C.c_double(0.0)
        P, lams = np.zeros((self.maxComponents, self._d)), np.zeros(self.maxComponents)
        capi.check(capi.lib().nfm_cfm_get_params(self._h, C.byref(nc), _vp(P), _vp(lams), _vp(self._w), C.byref(b)))
        self._P = np.ascontiguousarray(P.reshape(-1)[:nc.value * self._d].reshape(nc.value, self._d))
        self._lams = lams[:nc.value].copy()
        self._intercept = b.value
        self._dirty = False

    def init(self, X, force=False):
        """convex_factorization_machine.nim:49-60"""
        if force or not (self.warmStart and self.isInitialized):
            self._set(np.zeros((0, X.nFeatures)), np.zeros(0), np.zeros(X.nFeatures), 0.0)
        self.isInitialized = True

    def _set(self, P, lams, w, intercept):
        P = _f64(P)
        if self._d != P.shape[1]:
            self._release()
        self._d = P.shape[1]
        self.P, self.lams, self.w, self.intercept = P.copy(), _f64(lams).copy(), _f64(w).copy(), intercept

    def set_params(self, P, lams, w, intercept):
        """Inject parameters (what load does, convex_factorization_machine.nim:111-164)"""
        P, lams, w = _f64(P), _f64(lams), _f64(w)
        if P.ndim != 2 or P.shape[0] != len(lams) or len(lams) > self.maxComponents or len(w) != P.shape[1]:
            raise ValueError("P must have shape [len(lams), len(w)] with len(lams) <= maxComponents")
        self._set(P, lams, w, intercept)
        self.isInitialized = True

    def dump(self, fname):
        """convex_factorization_machine.nim:87-108: the reference's text format (ignoreDiag and warmStart are not stored)"""
        self.checkInitialized()
        nc, d = self._P.shape
        with open(os.path.expanduser(fname), "w") as f:
            f.write("task: %s\n" % self.task)
            f.write("nFeatures: %d\n" % d)
            f.write("degree: 2\n")
            f.write("nComponents: %d\n" % nc)
            f.write("maxComponents: %d\n" % self.maxComponents)
            f.write("fitIntercept: %s\n" % ("true" if self.fitIntercept else "false"))
            f.write("fitLinear: %s\n" % ("true" if self.fitLinear else "false"))
            f.write("lams:\n")
            f.write(_number_lines([self._lams]))
            f.write("P:\n")
            f.write(_number_lines(self._P[:nc]))
            f.write("w:\n")
            f.write(_number_lines([self._w]))
            f.write("intercept: %s\n" % _nim_float(self._intercept))


def _load_cfm(it, warmStart, ignoreDiag):
    """convex_factorization_machine.nim:111-164; it: the dump's lines (_DumpText)"""

    def field():
        return next(it).split(" ")[1]

    def truth(v):
        return v.lower() in ("true", "y", "yes", "1", "on")  # Nim's parseBool

    task = field()
    d = int(field())
    next(it)  # degree
    nc = int(field())
    max_components = int(field())
    fit_intercept, fit_linear = truth(field()), truth(field())
    cfm = ConvexFactorizationMachine(task, max_components, fit_intercept, fit_linear, bool(ignoreDiag), bool(warmStart))
    next(it)  # "lams:"
    lams = it.block(1, nc)
    lams = lams[0] if lams is not None else np.array(_floats(next(it))[:nc])
    next(it)  # "P:"
    P = np.zeros((nc, d))
    if it.block(nc, d, out=P) is None:
        for s_ in range(nc):
            P[s_] = _floats(next(it))[:d]
    next(it)  # "w:"
    w = it.block(1, d)
    w = w[0] if w is not None else np.array(_floats(next(it))[:d])
    intercept = float(next(it).split(" ")[1])
    cfm.set_params(P, lams, w, intercept)
    return cfm


def newConvexFactorizationMachine(task, maxComponents=30, fitIntercept=True, fitLinear=True, ignoreDiag=True, warmStart=False):
    """model/convex_factorization_machine.nim:25-46"""
    return ConvexFactorizationMachine(task, maxComponents, fitIntercept, fitLinear, ignoreDiag, warmStart)


def _refuse_convex(fm, solver):
    if isinstance(fm, ConvexFactorizationMachine):
        raise ValueError("%s does not fit a ConvexFactorizationMachine: newHazan(...).fit(X, y, cfm) and newGreedyCD(...).fit(X, y, cfm) do"
                         % solver)


def newFactorizationMachine(task, degree=2, nComponents=30, fitLower="explicit", fitIntercept=True, fitLinear=True,
                            warmStart=False, randomState=1, scale=0.01):
    return FactorizationMachine(task, degree, nComponents, fitLower, fitIntercept, fitLinear, warmStart, randomState,
                                scale)


def newFieldAwareFactorizationMachine(task, nComponents=10, fitIntercept=True, fitLinear=True, warmStart=False,
                                      randomState=1, scale=0.01):
    return FieldAwareFactorizationMachine(task, nComponents, fitIntercept, fitLinear, warmStart, randomState, scale)


# ------------------------------------------------------------------------------------------------
# loaders (dataset.nim:616-632, 768-790): text parsed on the GPU, the dataset stays in HBM
# ------------------------------------------------------------------------------------------------
def loadSVMLightFile(f, nFeatures=-1, ctx=None, layout="csr"):
    """-> (CSRDataset, y).  The reference fills `var dataset` / `var y` (dataset.nim:616-617).  layout="csc": -> (CSCDataset,
    y), the overload of dataset.nim:643-693 -- the same parse followed by the transposition on the device."""
    ctx = ctx or default_context()
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_load_svmlight(ctx.h, os.path.expanduser(f).encode(), int(nFeatures), C.byref(h)))
    ds = _as_layout(CSRDataset._from_loader(ctx, h), layout)
    return ds, ds.targets()


def loadFFMFile(f, nFeatures=-1, nFields=-1, ctx=None):
    """-> (CSRFieldDataset, y) (dataset.nim:768-790)."""
    ctx = ctx or default_context()
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_load_ffm(ctx.h, os.path.expanduser(f).encode(), int(nFeatures), int(nFields),
                                               C.byref(h)))
    ds = CSRDataset._from_loader(ctx, h)
    return ds, ds.targets()


def loadUserItemRatingFile(f, ctx=None, layout="csr"):
    """-> (CSRDataset, y) (dataset.nim:840-900): `user item rating [anything]` per line, any non-digit run a delimiter;
    row i = {user - minUser: 1, nUsers + item - minItem: 1}, parsed on the GPU.  layout="csc": -> (CSCDataset, y), the
    overload of dataset.nim:903-992 -- the same matrix by columns, with that overload's own line rule: lines of fewer than
    5 characters are skipped (:923, 955, 975), so a four-character line is skipped where the row-major loader refuses it."""
    ctx = ctx or default_context()
    if layout not in capi.LAYOUT:
        raise ValueError("layout must be one of %s" % sorted(capi.LAYOUT))
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_load_user_item_lines(ctx.h, os.path.expanduser(f).encode(), int(layout == "csc"), C.byref(h)))
    ds = _as_layout(CSRDataset._from_loader(ctx, h), layout)
    return ds, ds.targets()


def parseUserItemRatingText(text, ctx=None, layout="csr"):
    """loadUserItemRatingFile on an in-memory buffer (bytes)"""
    ctx = ctx or default_context()
    if layout not in capi.LAYOUT:
        raise ValueError("layout must be one of %s" % sorted(capi.LAYOUT))
    if isinstance(text, str):
        text = text.encode()
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_parse_user_item_lines(ctx.h, text, len(text), int(layout == "csc"), C.byref(h)))
    ds = _as_layout(CSRDataset._from_loader(ctx, h), layout)
    return ds, ds.targets()


# ------------------------------------------------------------------------------------------------
# datasets made from datasets on the device: shuffle, vstack, hstack, normalize
# ------------------------------------------------------------------------------------------------
def _resident(X, what):
    if not isinstance(X, CSRDataset):
        raise ValueError("%s needs a dataset resident on the device, not %s" % (what, type(X).__name__))
    return X


def shuffle(X, y, indices=None):
    """-> (X[indices], y[indices]) (dataset.nim:372-381); without indices the permutation is drawn from the global
    generator as dataset.nim:388-394 draws it (NimRand.shuffleForward)."""
    _row_major(_resident(X, "shuffle"), "shuffle (Accessing row vectors by openarray is not supported for CSCMatrix)")
    y = np.asarray(y)
    if len(y) != X.nSamples:
        raise ValueError("X.nSamples != len(y)")
    if indices is None:
        indices = np.arange(len(y), dtype=np.int64)
        globalRand().shuffleForward(indices)
    indices = _i64(indices)
    Xs = X[indices]  # checkIndicesRow first, as the reference's X[indices] does
    return Xs, y[indices]


def _stack(entry, parts, what):
    if len(parts) == 1 and isinstance(parts[0], (list, tuple)):
        parts = tuple(parts[0])
    if not parts:
        raise ValueError("%s needs at least one dataset" % what)
    for X in parts:
        _resident(X, what)
    if len({isinstance(X, CSCDataset) for X in parts}) > 1:
        raise ValueError("%s: row-major and column-major datasets cannot be stacked together (convert with toCSRDataset / "
                         "toCSCDataset)" % what)
    hs = (C.c_void_p * len(parts))(*[X.h for X in parts])
    h = C.c_void_p()
    capi.check(entry(hs, len(parts), C.byref(h)))
    return CSRDataset._from_loader(parts[0].ctx, h)


def vstack(*dataseq):
    """tensor/sparse.nim:564-581, 613-633; of CSCDatasets :583-610 (the result's indptr has nFeatures + 1 entries, not
    the shape[0] + 1 of :598)"""
    return _stack(capi.lib().nfm_dataset_vstack, dataseq, "vstack")


def hstack(*dataseq):
    """tensor/sparse.nim:671-698, 719-750; of CSCDatasets :701-716"""
    return _stack(capi.lib().nfm_dataset_hstack, dataseq, "hstack")


def normalize(X, axis=1, norm="l2"):
    """dataset.nim:398-403: in place, as the reference; returns None.  norm: "l1", "l2" or "linfty".  A CSCDataset:
    tensor/sparse.nim:414-427, the same fold with 1 - axis over the column arrays."""
    _resident(X, "normalize")
    if norm not in capi.NORM:
        raise ValueError("norm must be one of %s" % sorted(capi.NORM))
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_normalize(X.h, int(axis), capi.NORM[norm], C.byref(h)))
    X._swap_handle(h)


class StreamCSRDataset:
    """A STREAMCSR / STREAMCSRFIELD file used in row blocks (dataset.nim:170-174 newStreamCSRDataset(f, cacheSize);
    tensor/sparse_stream.nim:232-270 readCache): at most cacheRows rows are resident in HBM at a time.  fit walks the
    blocks in file order without shuffling, as the reference does for a dataset that is not fully cached
    (optimizer/sgd.nim:297, sgd_multi.nim:83-97)."""

    def __init__(self, f, cacheRows, ctx=None, fY=None):
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        capi.check(capi.lib().nfm_stream_open(self.ctx.h, os.path.expanduser(f).encode(),
                                              None if fY is None else os.path.expanduser(fY).encode(), C.byref(self.h)))
        n, d, nnz, nf = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        capi.check(capi.lib().nfm_stream_shape(self.h, C.byref(n), C.byref(d), C.byref(nnz), C.byref(nf)))
        self.nSamples, self._nFeatures, self.nnz, self.nFields = n.value, d.value, nnz.value, nf.value
        self.cacheRows = max(1, int(cacheRows))

    @property
    def nFeatures(self):
        return self._nFeatures

    @property
    def shape(self):
        return [self.nSamples, self._nFeatures]

    def blocks(self):
        return [(r0, min(self.nSamples, r0 + self.cacheRows)) for r0 in range(0, self.nSamples, self.cacheRows)]

    def prefetch(self, r0, r1):
        """starts loading rows [r0, r1) beside whatever runs on the context's stream (nfm_stream_prefetch_rows); the next
        load(r0, r1) hands the block over"""
        capi.check(capi.lib().nfm_stream_prefetch_rows(self.h, r0, r1))

    def load(self, r0, r1):
        """rows [r0, r1) as a resident dataset"""
        h = C.c_void_p()
        capi.check(capi.lib().nfm_stream_load_rows(self.h, r0, r1, C.byref(h)))
        return CSRDataset._from_loader(self.ctx, h)

    def __del__(self):
        try:
            if capi.alive and getattr(self, "h", None):
                capi.lib().nfm_stream_close(self.h)
                self.h = None
        except Exception:
            pass


def newStreamCSRDataset(f, fY=None, ctx=None, cacheRows=None):
    """dataset.nim:170-174 newStreamCSRDataset (+ loadStreamLabel, :1007-1014, when fY is given).  cacheRows = None:
    the STREAMCSR / STREAMCSRFIELD file is made resident in HBM as a whole; cacheRows = r: a StreamCSRDataset that
    keeps at most r rows resident per block (the reference's cacheSize, in rows; fit loads the next block while the
    current one trains, so two blocks are resident at a time).  -> (dataset, y)"""
    ctx = ctx or default_context()
    if cacheRows is not None:
        ds = StreamCSRDataset(f, cacheRows, ctx, fY)
        y = np.fromfile(os.path.expanduser(fY), dtype=np.float64) if fY is not None else np.zeros(ds.nSamples)
        if len(y) != ds.nSamples:
            raise ValueError("%s holds %d labels, the matrix has %d rows" % (fY, len(y), ds.nSamples))
        return ds, y
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_load_stream(ctx.h, os.path.expanduser(f).encode(),
                                                  None if fY is None else os.path.expanduser(fY).encode(), C.byref(h)))
    ds = CSRDataset._from_loader(ctx, h)
    return ds, ds.targets()


def convertSVMLightFile(fIn, fOutX, fOutY, ctx=None):
    """dataset.nim:1017-1097: svmlight text -> STREAMCSR binary + raw float64 labels"""
    ctx = ctx or default_context()
    capi.check(capi.lib().nfm_convert_svmlight(ctx.h, os.path.expanduser(fIn).encode(), os.path.expanduser(fOutX).encode(),
                                               os.path.expanduser(fOutY).encode()))


# ------------------------------------------------------------------------------------------------
# the binary stream files, written and transposed on the device
# ------------------------------------------------------------------------------------------------
def _path(f):
    return os.path.expanduser(f).encode()


def newStreamCSCDataset(f, fY=None, ctx=None):
    """dataset.nim:176-179 newStreamCSCDataset (+ loadStreamLabel, :1007-1014, when fY is given): the STREAMCSC file is made
    resident in HBM as a whole, as a CSCDataset with its row twin.  -> (dataset, y); y is zeros without fY"""
    ctx = ctx or default_context()
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_load_stream_csc(ctx.h, _path(f), None if fY is None else _path(fY), C.byref(h)))
    ds = CSRDataset._from_loader(ctx, h)
    return ds, ds.targets()


def transposeFile(fIn, fOut, cacheSize=200, ctx=None, chunkBytes=0):
    """dataset.nim:1100-1199: a STREAMCSR file -> the STREAMCSC file of the same matrix, or back; the header is copied as it
    is.  The result is the reference's at a cache that holds every entry; cacheSize is accepted and ignored (the whole
    matrix is resident on the device; with a smaller cache the reference's loop writes wrong files or raises).  A file
    whose first output record would be empty raises ValueError: the reference does not terminate on it."""
    ctx = ctx or default_context()
    capi.check(capi.lib().nfm_transpose_file(ctx.h, _path(fIn), _path(fOut), int(chunkBytes)))


def convertFFMFile(fIn, fOutX, fOutY, ctx=None):
    """dataset.nim:1202-1299: libffm text -> STREAMCSRFIELD binary + raw float64 labels.  ids are shifted by the smallest
    index seen, the fields are written as the text has them (the reference shifts only the ids), so only files with
    0-based fields reload through newStreamCSRDataset."""
    ctx = ctx or default_context()
    capi.check(capi.lib().nfm_convert_ffm(ctx.h, _path(fIn), _path(fOutX), _path(fOutY)))


def dumpStreamFile(f, X, chunkBytes=0):
    """X in the binary format that reloads by a plain upload: a CSRDataset -> STREAMCSR (field-aware: STREAMCSRFIELD), a
    CSCDataset -> STREAMCSC; packed on the device.  The targets are not part of the file."""
    _resident(X, "dumpStreamFile")
    capi.check(capi.lib().nfm_dataset_dump_stream(X.h, _path(f), int(chunkBytes)))


def formatStream(X, chunkBytes=0):
    """the bytes dumpStreamFile would write"""
    _resident(X, "formatStream")
    n = C.c_int64(0)
    capi.check(capi.lib().nfm_dataset_format_stream(X.h, int(chunkBytes), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    capi.check(capi.lib().nfm_dataset_format_stream(X.h, int(chunkBytes), buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def loadStreamLabel(fIn):
    """dataset.nim:1007-1014: the raw float64 values of a label file.  (The reference's two-argument form returns nSamples
    zeros followed by the values, :995-1004; it is not offered.)"""
    return np.fromfile(os.path.expanduser(fIn), dtype=np.float64)


def _dump_targets(X, y, what):
    """-> (y as float64 or None, y_int) for the dump entry points (dataset.nim:793-805: y is seq[float64] or seq[int])"""
    _row_major(_resident(X, what), what)
    if y is None:
        return None, 0
    y = np.asarray(y)
    if len(y) != X.nSamples:
        raise ValueError("X.nSamples != len(y).")
    y_int = int(np.issubdtype(y.dtype, np.integer) or y.dtype == np.bool_)
    return np.ascontiguousarray(y, dtype=np.float64), y_int


def dumpSVMLightFile(f, X, y=None, chunkBytes=0):
    """dataset.nim:793-805, formatted on the device.  y = None: the dataset's targets; an integer-typed y is written as
    integers ("1", "-1"), as the reference writes y: seq[int]."""
    y, y_int = _dump_targets(X, y, "dumpSVMLightFile")
    capi.check(capi.lib().nfm_dataset_dump_svmlight(X.h, os.path.expanduser(f).encode(), _vp(y), y_int, int(chunkBytes)))


def dumpFFMFile(f, X, y=None, chunkBytes=0):
    """dataset.nim:825-837, formatted on the device: "field:index:value" entries of a field-aware dataset"""
    y, y_int = _dump_targets(X, y, "dumpFFMFile")
    capi.check(capi.lib().nfm_dataset_dump_ffm(X.h, os.path.expanduser(f).encode(), _vp(y), y_int, int(chunkBytes)))


def formatText(X, y=None, chunkBytes=0):
    """the bytes dumpSVMLightFile / dumpFFMFile (for a field-aware X) would write: the counterpart of parseText"""
    y, y_int = _dump_targets(X, y, "formatText")
    n = C.c_int64(0)
    capi.check(capi.lib().nfm_dataset_format_text(X.h, _vp(y), y_int, int(chunkBytes), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    capi.check(capi.lib().nfm_dataset_format_text(X.h, _vp(y), y_int, int(chunkBytes), buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def parseText(text, withFields=False, nFeatures=-1, nFields=-1, ctx=None, layout="csr"):
    """the loaders on an in-memory buffer (bytes)"""
    ctx = ctx or default_context()
    if isinstance(text, str):
        text = text.encode()
    h = C.c_void_p()
    capi.check(capi.lib().nfm_dataset_parse_text(ctx.h, text, len(text), int(bool(withFields)), int(nFeatures),
                                                 int(nFields), C.byref(h)))
    ds = _as_layout(CSRDataset._from_loader(ctx, h), layout)
    return ds, ds.targets()


# ------------------------------------------------------------------------------------------------
# optimizers
# ------------------------------------------------------------------------------------------------
def _echo_header(maxIter, viol=True):
    """optimizer/utils.nim:26-40; viol = False: the solvers without a violation column (MBPSGD, PSGD)"""
    cols = ["Epoch".ljust(len(str(maxIter)))] + (["Violation".ljust(10)] if viol else []) + ["Loss".ljust(10), "Regularization"]
    print("   ".join(cols), flush=True)


def _echo_info(it, maxIter, viol, loss, regul):
    """optimizer/utils.nim:43-53; viol = None: no violation column (the reference passes -1)"""
    vals = ([] if viol is None else [viol]) + [loss, regul]
    print("   ".join([str(it).ljust(max(5, len(str(maxIter))))] + ["%-10.4e" % v for v in vals]), flush=True)


def _fit_prelude(X, y, model, handle, setTargets=True, colWise=None):
    """What every fit does between its own refusals and its loop: the target length check, set_targets (setTargets = False: a
    streamed dataset gets them block by block), the lookup of the device optimizer -- handle(), with whatever the solver settles
    from the data just before it -- and the push of a model that changed on the host.  -> (y as float64, handle's result)."""
    if colWise is None:  # every solver but the column-wise ones walks rows in storage order
        _row_major(X, "a row-wise solver")
    y = _f64(y)
    if len(y) != X.nSamples:
        raise ValueError("len(y) != nSamples")
    if setTargets:
        X.set_targets(y)  # checkTarget (fm_base.nim:29-36) is applied on the device from the model's task
    h = handle()
    if model._dirty:
        model._push(X.ctx)
    return y, h


class _IndexStream:
    """The sample indices the inner loops of MBPSGD and Katyusha consume, one chunk of `need` per outer iteration: `stream`
    if the caller gives one, else indices[ii] with wrap-around and reshuffle (minibatch_psgd.nim:98-108,169-170,
    katyusha.nim:108-118,199-200) -- rng.shuffle(indices) at the start and again the moment ii reaches n."""

    def __init__(self, n, need, shuffle, rng, stream=None):
        self.n, self.need, self.ii = n, need, 0
        self.rng = rng if shuffle and stream is None else None
        self.stream = None if stream is None else _i64(stream)
        self.indices = np.arange(n, dtype=np.int64)
        if self.rng is not None:
            self.rng.shuffle(self.indices)

    def chunk(self, it):
        need = self.need
        if self.stream is not None:
            chunk = self.stream[it * need:(it + 1) * need]
            if len(chunk) != need:
                raise ValueError("stream holds fewer than maxIter * miniBatchSize * maxIterInner indices")
            return chunk
        chunk = np.empty(need, dtype=np.int64)
        got = 0
        while got < need:
            take = min(need - got, self.n - self.ii)
            chunk[got:got + take] = self.indices[self.ii:self.ii + take]
            got += take
            self.ii += take
            if self.ii >= self.n:
                self.ii = 0
                if self.rng is not None:
                    self.rng.shuffle(self.indices)
        return chunk


def _default_batch(X):
    """minibatch_psgd.nim:160-163, katyusha.nim:203-206"""
    return max((X.nFeatures * X.nSamples) // max(X.nnz, 1), 1)


def _matrix_prox_reg(reg):
    """reg, or the reference's default newSquaredL12(); OmegaTI and OmegaCS have no matrix proximal operator (omegati.nim,
    omegacs.nim)"""
    reg = reg if reg is not None else newSquaredL12()
    if not isinstance(reg, (L1, L21, SquaredL12, SquaredL21)):
        raise ValueError("reg must be one of newL1(), newL21(), newSquaredL12(), newSquaredL21()")
    return reg


def _check_degree2(reg, fm):
    """initCD / initBCD / initSGD (squaredl12.nim:90-93,103-105, squaredl21.nim:69-70)"""
    if isinstance(reg, (SquaredL12, SquaredL21)) and fm.degree != 2:
        raise ValueError("%s supports only degree=2." % type(reg).__name__)


class _OptHandle:
    """The device optimizer (nfm_opt) a host optimizer owns: kept per (model, _params()), made by the subclass's _create(mh, out)."""
    _h = None
    _key = None

    def _handle(self, fm, ctx):
        mh = fm._push(ctx)
        key = (id(fm), mh.value, fm._gen) + self._params()
        if self._h is None or self._key != key:  # the device optimizer belongs to ONE device model
            self._release()
            self._h = C.c_void_p()
            capi.check(self._create(mh, C.byref(self._h)))
            self._key = key
        return self._h

    def _release(self):
        if self._h is not None and capi.alive:
            capi.lib().nfm_opt_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def _l2_penalty(fm, a0, a, b):
    """0.5 a0 b^2 + 0.5 a |w|^2 + 0.5 b |P|^2 (optimizer/utils.nim:56-59) on the host copy of the parameters"""
    return 0.5 * a0 * fm.intercept ** 2 + 0.5 * a * float((fm.w ** 2).sum()) + 0.5 * b * float((fm.P ** 2).sum())


def _reg_penalty(reg, gamma, fm, acc=0.0):
    """acc + gamma * reg.eval of every order, added one order after the other as the reference's loops do"""
    for order in range(fm.P.shape[0]):
        acc += gamma * reg.eval(np.ascontiguousarray(fm.P[order].T), fm.degree - order)
    return acc


class _OptimizerBase(_OptHandle):
    """optimizer/optimizer_base.nim:2-8 + the fit driver shared by SGD and AdaGrad."""

    def __init__(self, maxIter, alpha0, alpha, beta, loss, verbose, tol, shuffle, nCalls, mode, batch, lossParam,
                 deviceShuffle=False):
        if loss not in capi.LOSS:
            raise ValueError("unknown loss %r" % (loss,))
        if mode not in capi.MODE:
            raise ValueError("unknown mode %r" % (mode,))
        self.maxIter, self.alpha0, self.alpha, self.beta = int(maxIter), float(alpha0), float(alpha), float(beta)
        self.loss, self.lossParam = loss, float(lossParam)
        self.verbose, self.tol, self.shuffle, self.nCalls = int(verbose), float(tol), bool(shuffle), int(nCalls)
        self.mode, self.batch = mode, int(batch)
        # deviceShuffle (mini-batch mode): shuffle = true draws each epoch's order on the device (nfm_opt_set_shuffle) and
        # builds the next epoch's batch plan beside the current epoch, instead of shuffling `indices` on the host
        self.deviceShuffle = bool(deviceShuffle)
        self.it = 1
        self._model = None
        self._mode_built = None
        self._mh = None
        self.history = []  # (viol, mean loss) per epoch, what echoInfo prints
        self._dp = None  # (dp.Group, sync_period, overlap): see setDataParallel

    def _handle(self, fm, ctx, mode):
        mh = fm._push(ctx)
        key = (mode, self.batch) + self._cfg_key()  # a changed hyper-parameter needs a new device optimizer
        # the device optimizer belongs to ONE device model: a model that was released and created again (init /
        # set_params with another nFeatures) may sit at the same address -- compared by generation, not by pointer
        if self._h is None or self._model is not fm or self._mode_built != key or self._mh != (mh.value, fm._gen):
            self._release()
            self._h = C.c_void_p()
            self._create(mh, mode)
            self._model, self._mode_built, self._mh = fm, key, (mh.value, fm._gen)
            if self._dp is not None:
                self._attach_dp()
        return self._h

    def setDataParallel(self, group, syncPeriod=0, overlap=True, combine="auto"):
        """The maxThreads overloads across GPUs (optimizer/sgd_multi.nim:40-120 and twins): `group` is this rank's
        dp.Group; X handed to fit is then this rank's contiguous slice of the samples (dp.shard_bounds), every rank
        calls fit together, and the library reconciles the replicas every syncPeriod mini-batches (0: only at the end of
        every epoch).  AdaGrad's state increments are summed.  SGD: combine = "mean" (default) averages the ranks' increments
        (local SGD: as stable as one rank, the model moves as far as ONE rank's steps take it), "sum" adds them up (every
        rank's steps land in the model, as every Hogwild thread's steps do in the reference; acts like a step size times
        the number of ranks where features overlap -- keep syncPeriod small).  The epoch's loss / viol and the step
        counter `it` then cover the samples of ALL ranks."""
        if combine not in ("auto", "mean", "sum", "state_mean", "state_rsqrt", "state_cross"):
            raise ValueError("combine must be 'auto', 'mean', 'sum', 'state_mean', 'state_rsqrt' or 'state_cross'")
        # "auto" is resolved IN THE LIBRARY (NFM_DP_AUTO, the default of every optimizer -- the Nim and C++ hosts only call
        # nfm_opt_set_dp): what tools/dp_convergence.py measured: SGD -- the mean at any period; AdaGrad
        # -- the summed state is synchronous data-parallel AdaGrad when the ranks exchange after EVERY mini-batch and
        # over-shoots with longer periods, where the averaged state stays as stable as one rank
        self._dp = None if group is None else (group, int(syncPeriod), bool(overlap), combine)
        if self._h is not None:
            self._attach_dp()

    def _attach_dp(self):
        g = self._dp
        capi.check(capi.lib().nfm_opt_set_dp(self._h, None if g is None else g[0].h, 0 if g is None else g[1],
                                             1 if g is None or g[2] else 0))
        capi.check(capi.lib().nfm_opt_set_dp_combine(self._h, -1 if g is None else {"auto": -1, "mean": 0, "sum": 1, "state_mean": 2, "state_rsqrt": 3, "state_cross": 4}[g[3]]))

    def _sync_it(self):
        """with a group attached the library advances `it` by the samples of all ranks"""
        it = C.c_int64()
        capi.check(capi.lib().nfm_opt_get_it(self._h, C.byref(it)))
        self.it = it.value

    def _cfg_key(self):
        """what _create bakes into the device optimizer (the common part; subclasses extend it)"""
        return (self.alpha0, self.alpha, self.beta, self.loss, self.lossParam)

    def _restart_handle(self, fm, ctx, mode):
        """the step counter starts over unless the model is warm-started (sgd.nim:288-289, adagrad.nim:49-50), then the lookup"""
        if not fm.warmStart:
            self.it = 1
        return self._handle(fm, ctx, mode)

    def _epoch(self, X, perm, begin, end):
        ls, vs = C.c_double(0.0), C.c_double(0.0)
        capi.check(capi.lib().nfm_opt_epoch(self._h, X.h, _vp(perm), begin, end, C.byref(ls), C.byref(vs)))
        return ls.value, vs.value

    def _epoch_in_calls(self, X, perm, fm, callback):
        """one epoch as sub-range calls ending where it mod nCalls == 0, with finalize and the callback there (sgd.nim:303-308) -> sums"""
        n, pos, lossSum, violSum = X.nSamples, 0, 0.0, 0.0
        while pos < n:
            to_next = (self.nCalls - self.it % self.nCalls) % self.nCalls + 1
            end = min(n, pos + to_next)
            ls, vs = self._epoch(X, perm, pos, end)
            lossSum += ls
            violSum += vs
            self.it += end - pos
            pos = end
            if (self.it - 1) % self.nCalls == 0:
                self._finalize_into(fm)
                self.it -= 1  # the reference calls back before inc(self.it)
                callback(self, fm)
                self.it += 1
        return lossSum, violSum

    def last_permutation(self, n):
        """the sample order of the most recent permuted epoch call (nfm_opt_get_perm)"""
        out = np.zeros(n, dtype=np.int64)
        capi.check(capi.lib().nfm_opt_get_perm(self._h, _vp(out), n))
        return out

    def _finalize_into(self, fm):
        capi.check(capi.lib().nfm_opt_finalize(self._h))
        fm._pull()

    def _regularization(self, fm):
        """optimizer/utils.nim:56-59"""
        psq, wsq = C.c_double(0.0), C.c_double(0.0)
        capi.check(capi.lib().nfm_model_sqnorms(fm._h, C.byref(psq), C.byref(wsq)))
        b = C.c_double(0.0)
        return 0.5 * self.alpha * wsq.value + 0.5 * self.beta * psq.value  # intercept term added by caller

    def fit(self, X, y, fm, maxThreads=None, callback=None, perms=None, miniBatchSize=None, syncPeriod=None, devices=None):
        """optimizer/sgd.nim:261-328, adagrad.nim:137-203 (and the FFM / *_multi overloads).
        maxThreads (the reference's Hogwild overload) only SELECTS the mini-batch mode: a thread count is not a batch
        size.  The mode's knobs are explicit and defaulted: miniBatchSize (else the optimizer's `batch`, 8192),
        syncPeriod (mini-batches between exchanges of a data-parallel fit: setDataParallel, or `devices`), and
        devices = [ids]: ONE process trains over several GPUs (or one GPU listed several times) -- contiguous slices of
        the samples per device (optimizer/sgd_multi.nim:85-88), one replica + host thread each, reconciled by the library
        (nfm_dp_create_local).
        perms ([maxIter][n], optional) replaces the internal shuffle with explicit permutations: the
        reference shuffles with Nim's global RNG (sgd.nim:297), which a Nim host passes in here."""
        _refuse_convex(fm, type(self).__name__)
        _row_major(X, type(self).__name__)
        if devices is not None and len(devices) > 1:
            if perms is not None:
                raise ValueError("fit(devices=[...]) draws every rank's order itself (the device shuffle of its shard): perms is not supported")
            if isinstance(X, StreamCSRDataset):
                raise ValueError("fit(devices=[...]) needs a resident dataset (its rows are split over the devices), not a StreamCSRDataset")
            if callback is not None and self.nCalls > 0:
                raise ValueError("fit(devices=[...]) calls back once, after the fit: nCalls is not supported")
            return self._fit_devices(X, y, fm, list(devices), miniBatchSize, syncPeriod or 0, callback)
        if miniBatchSize is not None:  # for this fit only
            if int(miniBatchSize) < 1:
                raise ValueError("miniBatchSize < 1.")
            keep, self.batch = self.batch, int(miniBatchSize)
            try:
                return self.fit(X, y, fm, maxThreads, callback, perms, None, syncPeriod, None)
            finally:
                self.batch = keep
        if syncPeriod is not None and self._dp is not None:  # for this fit only, like miniBatchSize
            keep_dp, self._dp = self._dp, (self._dp[0], int(syncPeriod)) + tuple(self._dp[2:])
            if self._h is not None:
                self._attach_dp()
            try:
                return self.fit(X, y, fm, maxThreads, callback, perms, None, None, None)
            finally:
                self._dp = keep_dp
                if self._h is not None:
                    self._attach_dp()
        if isinstance(X, StreamCSRDataset):
            return self._fit_stream(X, y, fm, maxThreads, callback)
        fm.init(X)
        mode = self.mode if (maxThreads is None and self._dp is None) else "minibatch"
        y, _ = _fit_prelude(X, y, fm, lambda: self._restart_handle(fm, X.ctx, mode))
        capi.check(capi.lib().nfm_opt_set_it(self._h, self.it))
        dev_shuffle = self.shuffle and self.deviceShuffle and mode == "minibatch" and perms is None
        capi.check(capi.lib().nfm_opt_set_shuffle(self._h, int(getattr(fm, "randomState", 1)) if dev_shuffle else -1))
        if self.verbose > 0:
            _echo_header(self.maxIter)
        n = X.nSamples
        rng = globalRand()  # the reference shuffles with Nim's global generator, seeded by fm.init (sgd.nim:297)
        indices = np.arange(n, dtype=np.int64)
        isConverged = False
        per_epoch_cb = self._per_epoch_callback(callback)
        self.history = []
        # Host-side orders: epoch e+1's permutation is drawn while epoch e is still to run (the same sequence of shuffles
        # of the same array as the reference's, one epoch early) and announced to the library, which builds its batch
        # plan beside the running epoch (nfm_opt_announce_perm); two index arrays alternate.
        host_shuffle = self.shuffle and not dev_shuffle and perms is None
        order = [indices, None]
        if host_shuffle:
            rng.shuffle(order[0])  # sgd.nim:297 (Nim's global RNG there)
        whole_epochs = not (callback is not None and self.nCalls > 0 and mode == "sequential")
        if perms is not None:
            perms = [_i64(p_) for p_ in perms]
        for epoch in range(self.maxIter):
            viol = runningLoss = 0.0
            perm = nxt = None
            if perms is not None:
                perm = perms[epoch]
                nxt = perms[epoch + 1] if epoch + 1 < len(perms) and epoch + 1 < self.maxIter else None
            elif host_shuffle:
                perm = order[epoch % 2]
                if epoch + 1 < self.maxIter:
                    order[(epoch + 1) % 2] = perm.copy()
                    rng.shuffle(order[(epoch + 1) % 2])
                    nxt = order[(epoch + 1) % 2]
            if nxt is not None and whole_epochs and mode == "minibatch":
                capi.check(capi.lib().nfm_opt_announce_perm(self._h, _vp(nxt), 0, n))
            if callback is not None and self.nCalls > 0 and mode == "sequential":
                runningLoss, viol = self._epoch_in_calls(X, perm, fm, callback)
            else:
                runningLoss, viol = self._epoch(X, perm, 0, n)
                self.it += n
            n_all = n
            if self._dp is not None:  # sums and step counter cover all ranks' samples
                it0 = self.it - n
                self._sync_it()
                n_all = self.it - it0
            runningLoss /= float(n_all)
            if per_epoch_cb:
                self._finalize_into(fm)
                callback(self, fm)
            self.history.append((viol, runningLoss))
            # stoppingCriterion, sgd.nim:72-89
            isContinue = True
            if math.isnan(runningLoss):
                print("Loss is NaN. Use smaller learning rate.")
                isContinue = False
            if self.verbose > 0:
                b = C.c_double(0.0)
                reg = self._regularization(fm)
                capi.check(capi.lib().nfm_model_get_params(fm._h, None, None, C.byref(b)))
                _echo_info(epoch + 1, self.maxIter, viol, runningLoss, reg + 0.5 * self.alpha0 * b.value ** 2)
            if viol < self.tol:
                if self.verbose > 0:
                    print("Converged at epoch %d." % epoch)
                isConverged = True
                isContinue = False
            if not isContinue:
                break
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        self._finalize_into(fm)
        return self


def _fit_devices(self, X, y, fm, devices, miniBatchSize, syncPeriod, callback):
    """fit(..., devices=[...]): the maxThreads overloads over several GPUs from ONE process.  Rank r gets the contiguous
    slice dp.shard_bounds(n, r, world) of the samples on devices[r] (the reference's thread partition,
    optimizer/sgd_multi.nim:85-88), its own replica of `fm` and of this optimizer, and a host thread; the library
    reconciles the replicas every syncPeriod mini-batches and exactly at the end of every epoch (nfm_dp_create_local).
    All replicas end bitwise identical; rank 0's comes back in `fm`, its history / step counter in `self`."""
    import copy
    import threading

    from . import dp

    fm.init(X)
    y = _f64(y)
    n, world = X.nSamples, len(devices)
    if len(y) != n:
        raise ValueError("len(y) != nSamples")
    indptr, indices, data, fields = X.to_host()
    ctxs = [Context(int(d_)) for d_ in devices]
    groups = dp.Group.local(ctxs)
    P0, w0, b0 = np.array(fm.P), np.array(fm.w), float(fm.intercept)
    models, opts, err = [None] * world, [None] * world, []

    def body(r):
        try:
            lo, hi = dp.shard_bounds(n, r, world)
            a, b = int(indptr[lo]), int(indptr[hi])
            if fields is not None:
                Xr = newCSRFieldDataset(data[a:b], indices[a:b], indptr[lo:hi + 1] - a, fields[a:b], hi - lo, X.nFeatures, X.nFields, ctx=ctxs[r])
            else:
                Xr = newCSRDataset(data[a:b], indices[a:b], indptr[lo:hi + 1] - a, hi - lo, X.nFeatures, ctx=ctxs[r])
            fr = copy.copy(fm)
            fr._h, fr._ctx, fr._dirty = None, None, True  # a replica of its own on this rank's device
            fr.warmStart = True
            fr.set_params(P0, w0, b0)
            orr = copy.copy(self)
            orr._h, orr._model, orr._mode_built, orr._mh, orr.history = None, None, None, None, []
            if miniBatchSize is not None:
                orr.batch = int(miniBatchSize)
            orr.setDataParallel(groups[r], syncPeriod=syncPeriod)
            orr.fit(Xr, y[lo:hi], fr, maxThreads=world, callback=None)
            models[r], opts[r] = fr, orr
        except BaseException as e:  # noqa: BLE001
            err.append((r, e))

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for g in groups:
        g.close()
    if err:
        raise err[0][1]
    fm.set_params(models[0].P, models[0].w, models[0].intercept)
    self.it, self.history = opts[0].it, list(opts[0].history)
    if callback is not None:  # ONCE, with the finished model (the ranks train without a host in their epoch loops)
        callback(self, fm)
    return self


def _fit_stream(self, X, y, fm, maxThreads=None, callback=None):
    """fit over a dataset that is resident one row block at a time (optimizer/sgd_multi.nim:83-97: `while nRest > 0:
    X.readCache(...)`): blocks in file order, no shuffling (sgd.nim:297 shuffles only a fully cached dataset); the
    optimizer's step counter, scales and state continue from block to block."""
    fm.init(X)
    mode = self.mode if (maxThreads is None and self._dp is None) else "minibatch"
    y, _ = _fit_prelude(X, y, fm, lambda: self._restart_handle(fm, X.ctx, mode), setTargets=False)  # (targets: block by block)
    capi.check(capi.lib().nfm_opt_set_it(self._h, self.it))
    capi.check(capi.lib().nfm_opt_set_shuffle(self._h, -1))
    if self.verbose > 0:
        _echo_header(self.maxIter)
    n = X.nSamples
    isConverged = False
    self.history = []
    blocks = X.blocks()
    for epoch in range(self.maxIter):
        viol = runningLoss = 0.0
        for bi, (r0, r1) in enumerate(blocks):
            blk = X.load(r0, r1)
            if len(blocks) > 1 and os.environ.get("NIMFM_STREAM_PREFETCH", "1") != "0":  # the next block (the next epoch's first one after the last) is read, uploaded and split
                X.prefetch(*blocks[(bi + 1) % len(blocks)])  # while this one trains: two blocks resident at a time
            blk.set_targets(y[r0:r1])
            ls, vs = self._epoch(blk, None, 0, r1 - r0)
            runningLoss += ls
            viol += vs
            self.it += r1 - r0
            del blk
        runningLoss /= float(n)
        if callback is not None:
            self._finalize_into(fm)
            callback(self, fm)
        self.history.append((viol, runningLoss))
        isContinue = True
        if math.isnan(runningLoss):
            print("Loss is NaN. Use smaller learning rate.")
            isContinue = False
        if self.verbose > 0:
            b = C.c_double(0.0)
            reg = self._regularization(fm)
            capi.check(capi.lib().nfm_model_get_params(fm._h, None, None, C.byref(b)))
            _echo_info(epoch + 1, self.maxIter, viol, runningLoss, reg + 0.5 * self.alpha0 * b.value ** 2)
        if viol < self.tol:
            if self.verbose > 0:
                print("Converged at epoch %d." % epoch)
            isConverged = True
            isContinue = False
        if not isContinue:
            break
    if not isConverged and self.verbose > 0:
        print("Objective did not converge. Increase maxIter.")
    self._finalize_into(fm)
    return self


_OptimizerBase._fit_stream = _fit_stream
_OptimizerBase._fit_devices = _fit_devices


class SGD(_OptimizerBase):
    def __init__(self, maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared",
                 scheduling="optimal", power=1.0, verbose=1, tol=1e-3, shuffle=True, nCalls=-1, mode="sequential",
                 batch=8192, lossParam=1.0, deviceShuffle=False, touchCap=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, shuffle, nCalls, mode, batch, lossParam, deviceShuffle)
        if scheduling not in capi.SCHED:
            raise ValueError("unknown scheduling %r" % (scheduling,))
        self.eta0, self.scheduling, self.power = float(eta0), scheduling, float(power)
        # mini-batch mode: how many of a batch's per-sample steps on one coordinate are summed before averaging sets in
        # (nfm_opt_set_touch_cap; 1 = the per-coordinate mean; the reference's Hogwild with T threads ~ T)
        if not float(touchCap) >= 1.0:
            raise ValueError("touchCap < 1.")
        self.touchCap = float(touchCap)

    def _create(self, mh, mode):
        cfg = capi.SGDCfg(self.eta0, self.alpha0, self.alpha, self.beta, self.power, self.lossParam,
                          capi.LOSS[self.loss], capi.SCHED[self.scheduling], capi.MODE[mode], 0, self.batch)
        capi.check(capi.lib().nfm_sgd_create(mh, C.byref(cfg), C.byref(self._h)))
        if mode == "minibatch" and self.touchCap != 1.0:
            capi.check(capi.lib().nfm_opt_set_touch_cap(self._h, self.touchCap))

    def _cfg_key(self):
        return super()._cfg_key() + (self.eta0, self.scheduling, self.power, self.touchCap)

    def _per_epoch_callback(self, callback):
        return callback is not None and (self.nCalls <= 0 or self.mode != "sequential")  # sgd.nim:312


class AdaGrad(_OptimizerBase):
    def __init__(self, maxIter=100, eta0=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared", eps=1e-10,
                 verbose=1, tol=1e-3, shuffle=True, nCalls=-1, mode="sequential", batch=8192, lossParam=1.0,
                 trackViol=True, deviceShuffle=False, adaCross=0.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, shuffle, nCalls, mode, batch, lossParam, deviceShuffle)
        self.eta0, self.eps, self.trackViol = float(eta0), float(eps), bool(trackViol)
        # mini-batch mode: the weight of the batch's gradient cross products in g_norm (nfm_opt_set_ada_cross; 0 = the samples'
        # squares alone; 0.1 lets field-aware AdaGrad run at batch 32768 with the epochs-to-target of batch 2048)
        if not float(adaCross) >= 0.0:
            raise ValueError("adaCross < 0.")
        self.adaCross = float(adaCross)

    def _create(self, mh, mode):
        cfg = capi.AdaGradCfg(self.eta0, self.alpha0, self.alpha, self.beta, self.eps, self.lossParam,
                              capi.LOSS[self.loss], capi.MODE[mode], int(self.trackViol), 0, self.batch)
        capi.check(capi.lib().nfm_adagrad_create(mh, C.byref(cfg), C.byref(self._h)))
        if mode == "minibatch" and self.adaCross != 0.0:
            capi.check(capi.lib().nfm_opt_set_ada_cross(self._h, self.adaCross))

    def _cfg_key(self):
        return super()._cfg_key() + (self.eta0, self.eps, self.trackViol, self.adaCross)

    def _per_epoch_callback(self, callback):
        return callback is not None  # adagrad.nim:188-191

    def get_state(self, fm):
        """g_sum / g_norm (adagrad.nim:15-16) in the reference layout."""
        nb, da, k = (fm._P.shape[0], fm._P.shape[2], fm._P.shape[1]) if isinstance(fm, FactorizationMachine) else (
            fm._P.shape[0], fm._P.shape[1], fm._P.shape[2])
        gs, gn = np.zeros((nb, da, k)), np.zeros((nb, da, k))
        gsw, gnw = np.zeros(len(fm._w)), np.zeros(len(fm._w))
        gsb, gnb = C.c_double(0.0), C.c_double(0.0)
        capi.check(capi.lib().nfm_opt_get_state(self._h, _vp(gs), _vp(gn), _vp(gsw), _vp(gnw), C.byref(gsb),
                                                C.byref(gnb)))
        return gs, gn, gsw, gnw, gsb.value, gnb.value


def suggestTouchCap(X, batch):
    """A touch cap for `newSGD(mode="minibatch", batch=batch, touchCap=...)` on dataset X (anything with nSamples, nFeatures,
    nnz): about twice the mean number of a batch's samples that touch one coordinate, lambda = batch * (entries per row) /
    nFeatures, as a power of two between 16 and 64 -- the settings measured to keep the epochs to a held-out loss of the
    reference's sample order (profiles/r05h_touch_cap_sweep.txt: 16 up to lambda ~ 10, 32 at 17-21,
    64 at 34).  Not a default: the library's own default stays 1, the per-coordinate mean (include/nimfm_hip.h)."""
    n, d, nnz = int(X.nSamples), int(X.nFeatures), int(X.nnz)
    if n <= 0 or d <= 0 or int(batch) < 1:
        raise ValueError("suggestTouchCap: empty dataset or batch < 1.")
    lam = min(int(batch), n) * (nnz / n) / d
    cap = 16.0
    while cap < 64.0 and 2.0 * lam > cap * 2.0 ** 0.5:  # (to the nearest power of two in the logarithm)
        cap *= 2.0
    return cap


def newSGD(maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared", scheduling="optimal",
           power=1.0, verbose=1, tol=1e-3, shuffle=True, nCalls=-1, **gpu):
    return SGD(maxIter, eta0, alpha0, alpha, beta, loss, scheduling, power, verbose, tol, shuffle, nCalls, **gpu)


def newAdaGrad(maxIter=100, eta0=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared", eps=1e-10, verbose=1,
               tol=1e-3, shuffle=True, nCalls=-1, **gpu):
    return AdaGrad(maxIter, eta0, alpha0, alpha, beta, loss, eps, verbose, tol, shuffle, nCalls, **gpu)


# ------------------------------------------------------------------------------------------------
# coordinate descent (optimizer/cd.nim)
# ------------------------------------------------------------------------------------------------
class _WholeIterSolver(_OptHandle):
    """What the solvers that run one whole iteration per nfm_opt_epoch call share: the CD family and the PGD family.  The
    device optimizer is kept per (model, hyper-parameters) -- it carries the cached schedule (CD) or t, c, q and the caches
    of a warm-started fit (FISTA, NMAPGD).  The iteration loop, the stopping rule, the verbose lines and the callback run
    here where the reference has them.  A subclass supplies _params, _create, _begin_fit and _reg_value, and _iteration
    where an iteration records more than (viol, mean loss); Katyusha, whose iteration walks an index stream, also _resolve and
    _chunks."""
    _name = None
    _callback_first = True  # the callback before the verbose line, or after it
    _nan_stops = False  # "Loss is NaN" ends the fit, between the callback and the verbose line
    _resident_note = ""
    _col_wise = None  # True: the reference's fit takes a ColDataset (the CD family), so a CSCDataset is accepted

    def __init__(self, maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam):
        if loss not in capi.LOSS:
            raise ValueError("unknown loss %r" % (loss,))
        self.maxIter, self.alpha0, self.alpha, self.beta = int(maxIter), float(alpha0), float(alpha), float(beta)
        self.loss, self.lossParam, self.verbose, self.tol = loss, float(lossParam), int(verbose), float(tol)
        self.history = []  # one tuple per iteration, what echoInfo prints

    def _check(self, fm):
        pass

    def _resolve(self, X, fm):
        """what the fit settles from the data once the inputs are checked, before the device optimizer is looked up"""

    def _chunks(self, X, stream):
        """called before the header -> the function that gives (perm, begin, end) of iteration `it`: all samples in order"""
        return lambda it: (None, 0, X.nSamples)

    def _iteration(self, ls, vs, n):
        self.history.append((vs, ls / float(n)))
        return self.history[-1]

    def _reset_records(self):
        self.history = []

    def _converged_label(self, it):
        return "iteration %d" % (it + 1)

    def fit(self, X, y, fm, callback=None):
        """cd.nim:128-186, pcd.nim:110-201, pbcd.nim:212-329; pgd.nim:149-217, fista.nim:52-141, nmapgd.nim:174-268"""
        return self._fit(X, y, fm, callback, None)

    def _fit(self, X, y, fm, callback, stream):
        _refuse_convex(fm, self._name)
        if not isinstance(fm, FactorizationMachine):
            raise ValueError("%s fits a FactorizationMachine" % self._name)
        if isinstance(X, StreamCSRDataset):
            raise ValueError("%s needs a resident dataset%s" % (self._name, self._resident_note))
        fm.init(X)
        self._check(fm)

        def handle():
            self._resolve(X, fm)
            return self._handle(fm, X.ctx)

        y, h = _fit_prelude(X, y, fm, handle, colWise=self._col_wise)
        capi.check(self._begin_fit(h, X, fm))
        n = X.nSamples
        chunk_of = self._chunks(X, stream)
        if self.verbose > 0:
            _echo_header(self.maxIter)
        self._reset_records()
        isConverged = False
        for it in range(self.maxIter):
            ls, vs = C.c_double(0.0), C.c_double(0.0)
            perm, begin, end = chunk_of(it)
            capi.check(capi.lib().nfm_opt_epoch(h, X.h, _vp(perm), begin, end, C.byref(ls), C.byref(vs)))
            viol, lossVal = self._iteration(ls.value, vs.value, n)
            if callback is not None and self._callback_first:
                fm._pull()
                callback(self, fm)
            if self._nan_stops and math.isnan(lossVal):
                print("Loss is NaN. Use smaller learning rate.")
                break
            if self.verbose > 0:
                _echo_info(it + 1, self.maxIter, viol, lossVal, self._reg_value(fm, n))
            if callback is not None and not self._callback_first:
                fm._pull()
                callback(self, fm)
            if viol < self.tol:
                if self.verbose > 0:
                    print("Converged at %s." % self._converged_label(it))
                isConverged = True
                break
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        fm._pull()
        return self


class CD(_WholeIterSolver):
    """optimizer/cd.nim:6-25,128-186: newCD(...).fit(X, y, fm).  The caches, the level schedule and every iteration run on
    the device (nfm_cd_create / nfm_cd_begin_fit / nfm_opt_epoch).  The reference fits a ColDataset; the library builds the
    column twin of the row dataset itself (once per dataset).  history: (viol, mean loss) per iteration."""
    _name = "CD"
    _callback_first = True  # cd.nim: the callback before the verbose line; pcd.nim:188-192 after it
    _resident_note = " (the reference's fit takes a ColDataset)"
    _col_wise = True

    def __init__(self, maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared", verbose=1, tol=1e-3, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)

    def _params(self):
        return (self.alpha0, self.alpha, self.beta, self.loss, self.lossParam)

    def _create(self, mh, out):
        return capi.lib().nfm_cd_create(mh, self.alpha0, self.alpha, self.beta, capi.LOSS[self.loss], self.lossParam, out)

    def _begin_fit(self, h, X, fm):
        return capi.lib().nfm_cd_begin_fit(h, X.h)

    def schedule(self, X, fm):
        """(number of levels, widest level) of the P sweep's schedule on X (nfm_cd_schedule); fm must be initialised"""
        fm.checkInitialized()
        h = self._handle(fm, X.ctx)
        lv, wd = C.c_int64(0), C.c_int64(0)
        capi.check(capi.lib().nfm_cd_schedule(h, X.h, C.byref(lv), C.byref(wd)))
        return lv.value, wd.value

    def _reg_value(self, fm, n):
        fm._pull()  # the penalty is computed here, from the host copy
        nd = float(n)
        return self._penalty(fm, nd) / nd

    def _penalty(self, fm, nd):
        """the verbose line's regularisation times nSamples (cd.nim:176-184): the SCALED strengths"""
        return _l2_penalty(fm, self.alpha0 * nd, self.alpha * nd, self.beta * nd)


def newCD(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-3, loss="squared", verbose=1, tol=1e-3, lossParam=1.0):
    """optimizer/cd.nim:12-25 (lossParam: the Huber threshold, newHuber(threshold))"""
    return CD(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)


class PCD(CD):
    """optimizer/pcd.nim:9-35,110-201: newPCD(...).fit(X, y, sfm).  CD's device iteration with a proximal step per
    feature (nfm_pcd_create): L1 and row-wise SquaredL12 keep CD's level schedule, column-wise SquaredL12 (the default)
    and OmegaTI a run schedule.  The loop, the stopping rule, the verbose lines and the callback run
    here where the reference has them."""

    def __init__(self, maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, verbose=1,
                 tol=1e-3, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)
        self.gamma = float(gamma)
        self.reg = reg if reg is not None else newSquaredL12()
        if not isinstance(self.reg, (L1, SquaredL12, OmegaTI)):
            if isinstance(self.reg, (L21, SquaredL21)):  # nimfm_sparsefm.nim:124-146
                raise ValueError("PCD cannot be used for %s." % ("L21" if isinstance(self.reg, L21) else "squaredL21"))
            raise ValueError("reg must be one of newL1(), newSquaredL12(), newOmegaTI()")

    _name = "PCD"
    _callback_first = False

    def _params(self):
        return super()._params() + (self.gamma, self.reg.name, self.reg.transpose)

    def _create(self, mh, out):
        return capi.lib().nfm_pcd_create(mh, self.alpha0, self.alpha, self.beta, self.gamma, capi.LOSS[self.loss], self.lossParam,
                                         capi.REG[self.reg.name], int(self.reg.transpose), out)

    def _check(self, sfm):
        _check_degree2(self.reg, sfm)

    def _penalty(self, sfm, nd):
        """pcd.nim:176-189: gamma * n * reg.eval per order, then CD's scaled L2 terms"""
        return _reg_penalty(self.reg, self.gamma * nd, sfm) + super()._penalty(sfm, nd)

    def schedule(self, X, fm):
        """(number of levels or runs, widest) of the P sweep's schedule on X (nfm_cd_schedule): runs for column-wise
        SquaredL12 and OmegaTI, levels otherwise"""
        return super().schedule(X, fm)


def newPCD(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, verbose=1, tol=1e-3,
           lossParam=1.0):
    """optimizer/pcd.nim:17-35; reg=None is newSquaredL12() (column-wise), the reference's default"""
    return PCD(maxIter, alpha0, alpha, beta, gamma, loss, reg, verbose, tol, lossParam)


class PBCD(CD):
    """optimizer/pbcd.nim:8-46,212-329: newPBCD(...).fit(X, y, sfm) at maxSearch = 0.  A feature's whole row of P steps at
    once (nfm_pbcd_create): L1 and L21 on CD's level schedule, SquaredL21 (the default) and OmegaCS (at any degree) on the
    run schedule.  beta and gamma are not scaled by nSamples here (pbcd.nim:138,147,154).  The loop, the stopping rule, the
    verbose lines and the callback run here where the reference has them."""

    def __init__(self, maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, verbose=1,
                 tol=1e-3, sigma=0.01, rho=0.5, maxSearch=0, shrink=False, shuffle=False, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)
        self.gamma = float(gamma)
        self.reg = reg if reg is not None else newSquaredL21()
        self.sigma, self.rho, self.maxSearch = float(sigma), float(rho), int(maxSearch)
        self.shrink, self.shuffle = bool(shrink), bool(shuffle)  # shrink: stored and never read (pbcd.nim:16)
        if isinstance(self.reg, SquaredL12):  # nimfm_sparsefm.nim:118
            raise ValueError("PBCD cannot be used for squaredl12.")
        if not isinstance(self.reg, (L1, L21, SquaredL21, OmegaCS)):
            raise ValueError("reg must be one of newL1(), newL21(), newSquaredL21(), newOmegaCS()")
        if isinstance(self.reg, SquaredL21) and self.reg.transpose:  # initBCD, squaredl21.nim:71-72
            raise ValueError("transpose=true is not supported for BCD.")
        if self.maxSearch != 0:  # the acceptance test reads a loss total accumulated feature by feature over the sweep
            raise ValueError("maxSearch != 0 (the line search, pbcd.nim:80-109) is not supported")
        if self.shuffle:  # pbcd.nim:172 draws from Nim's global generator
            raise ValueError("shuffle=True is not supported: the features step in the schedule's order")

    _name = "PBCD"
    _callback_first = False  # pbcd.nim:302-314: the verbose line, then the callback

    def _params(self):
        return super()._params() + (self.gamma, self.reg.name, self.maxSearch)

    def _create(self, mh, out):
        return capi.lib().nfm_pbcd_create(mh, self.alpha0, self.alpha, self.beta, self.gamma, capi.LOSS[self.loss], self.lossParam,
                                          capi.REG[self.reg.name], self.maxSearch, out)

    def _check(self, sfm):
        _check_degree2(self.reg, sfm)

    def _penalty(self, sfm, nd):
        """pbcd.nim:303-306 (regularization, optimizer/utils.nim, with the UNSCALED strengths), times nSamples as the
        shared loop divides by it"""
        return _reg_penalty(self.reg, self.gamma, sfm, _l2_penalty(sfm, self.alpha0, self.alpha, self.beta)) * nd

    def schedule(self, X, fm):
        """(number of levels or runs, widest) of the P sweep's schedule on X (nfm_cd_schedule): runs for SquaredL21 and
        OmegaCS, levels for L1 and L21"""
        return super().schedule(X, fm)


def newPBCD(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, verbose=1, tol=1e-3,
            sigma=0.01, rho=0.5, maxSearch=0, shrink=False, shuffle=False, lossParam=1.0):
    """optimizer/pbcd.nim:20-46; reg=None is newSquaredL21(), the reference's default"""
    return PBCD(maxIter, alpha0, alpha, beta, gamma, loss, reg, verbose, tol, sigma, rho, maxSearch, shrink, shuffle, lossParam)


# ------------------------------------------------------------------------------------------------
# mini-batch proximal SGD
# ------------------------------------------------------------------------------------------------
class _Regularizer:
    """regularizer/*.nim: the sparsity-inducing penalties that have a matrix proximal operator.
    eval (for the verbose line, minibatch_psgd.nim:196-199) runs on the host copy of one order, [d+a][k]."""
    name = None

    def __init__(self, transpose=False):
        self.transpose = bool(transpose)


class L1(_Regularizer):
    name = "l1"

    def eval(self, Pt, degree=2):  # l1.nim:19-22
        return float(np.abs(Pt).sum())


class L21(_Regularizer):
    name = "l21"

    def eval(self, Pt, degree=2):  # l21.nim:17-20
        return float(np.sqrt((Pt * Pt).sum(1)).sum())


class SquaredL12(_Regularizer):
    name = "squaredl12"

    def __init__(self, transpose=True):  # squaredl12.nim:85-88
        super().__init__(transpose)

    def eval(self, Pt, degree=2):  # squaredl12.nim:72-82
        if degree > 2:
            raise ValueError("SquaredL12 supports only degree=2.")
        return float((np.abs(Pt).sum(0 if self.transpose else 1) ** 2).sum())


class SquaredL21(_Regularizer):
    name = "squaredl21"

    def __init__(self, transpose=False):  # squaredl21.nim:15-17
        super().__init__(transpose)

    def eval(self, Pt, degree=2):  # squaredl21.nim:21-29
        if degree != 2:
            raise ValueError("SquaredL21 supports only degree=2.")
        return float(np.sqrt((Pt * Pt).sum(0 if self.transpose else 1)).sum() ** 2)


def newL1():
    return L1()


def newL21():
    return L21()


def newSquaredL12(transpose=True):
    return SquaredL12(transpose)


def newSquaredL21(transpose=False):
    return SquaredL21(transpose)


class OmegaTI(_Regularizer):
    """regularizer/omegati.nim: the ANOVA-kernel penalty over |P|.  It has no matrix proximal operator, so MBPSGD refuses it;
    PCD takes it (omegati.nim:33-66)."""
    name = "omegati"

    def __init__(self):
        super().__init__(False)

    def eval(self, Pt, degree=2):  # omegati.nim:17-26, Pt: [nFeatures][nComponents]
        Pt = np.asarray(Pt, dtype=np.float64)
        cache = np.zeros((degree + 1, Pt.shape[1]))
        cache[0] = 1.0
        for j in range(Pt.shape[0]):
            a = np.abs(Pt[j])
            for deg in range(degree):
                cache[degree - deg] += cache[degree - deg - 1] * a
        return float(sum(cache[degree]))


def newOmegaTI():
    return OmegaTI()


class OmegaCS(_Regularizer):
    """regularizer/omegacs.nim: the ANOVA-kernel penalty over the norms of P's rows (feature selection).  It has BCD hooks
    only (omegacs.nim:31-85): PBCD takes it, at any degree; PCD and the matrix-prox solvers refuse it."""
    name = "omegacs"

    def __init__(self):
        super().__init__(False)

    def eval(self, Pt, degree=2):  # omegacs.nim:15-28 with recomputeCacheBCD's loop order (:42-44), Pt: [nFeatures][nComponents]
        Pt = np.asarray(Pt, dtype=np.float64)
        cache = [0.0] * (degree + 1)
        cache[0] = 1.0
        for nj in np.sqrt((Pt * Pt).sum(1)).tolist():
            for deg in range(degree):
                cache[degree - deg] += cache[degree - deg - 1] * nj
        return float(cache[degree])


def newOmegaCS():
    return OmegaCS()


class MBPSGD(_OptimizerBase):
    """optimizer/minibatch_psgd.nim:11-65,125-210: newMBPSGD(...).fit(X, y, sfm).  The gradient of a mini-batch,
    the step on all parameters and the proximal operator run on the device (nfm_mbpsgd_create / nfm_opt_epoch);
    the outer loop, the index stream (indices[ii] with wrap-around and reshuffle, :98-108), the stopping rule
    (:201-204) and the verbose lines run here where the reference has them."""

    def __init__(self, maxIter=100, eta0=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None,
                 miniBatchSize=-1, maxIterInner=-1, scheduling="optimal", power=1.0, verbose=1, tol=1e-6, shuffle=True,
                 nCalls=-1, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, shuffle, nCalls, "minibatch", 1, lossParam)
        if scheduling not in capi.SCHED:
            raise ValueError("unknown scheduling %r" % (scheduling,))
        self.reg = _matrix_prox_reg(reg)
        self.gamma, self.eta0, self.scheduling, self.power = float(gamma), float(eta0), scheduling, float(power)
        self.miniBatchSize, self.maxIterInner = int(miniBatchSize), int(maxIterInner)
        self.it = 0  # :63

    def _create(self, mh, mode):
        cfg = capi.MBPSGDCfg(self.eta0, self.alpha0, self.alpha, self.beta, self.gamma, self.power, self.lossParam,
                             capi.LOSS[self.loss], capi.SCHED[self.scheduling], capi.REG[self.reg.name],
                             int(self.reg.transpose), self.batch)
        capi.check(capi.lib().nfm_mbpsgd_create(mh, C.byref(cfg), C.byref(self._h)))

    def _cfg_key(self):
        return super()._cfg_key() + (self.eta0, self.gamma, self.scheduling, self.power, self.reg.name, self.reg.transpose)

    def fit(self, X, y, sfm, callback=None, stream=None):
        """stream (optional): the sample indices in the order the inner loops consume them, at least
        maxIter * miniBatchSize * maxIterInner of them -- replaces the internal shuffle (Nim's global RNG in the
        reference, :107,170), which a Nim host passes in here."""
        _refuse_convex(sfm, "MBPSGD")
        if not isinstance(sfm, FactorizationMachine):
            raise ValueError("MBPSGD fits a FactorizationMachine")
        sfm.init(X)
        n = X.nSamples
        B = self.miniBatchSize if self.miniBatchSize > 0 else _default_batch(X)  # :160-163
        inner = self.maxIterInner
        if inner <= 0:  # :164-167
            inner = max((n - 1) // B + 1, 1)

        def handle():
            if not sfm.warmStart:
                self.it = 1  # :153-154
            _check_degree2(self.reg, sfm)
            self.batch = B
            return self._handle(sfm, X.ctx, "minibatch")

        y, _ = _fit_prelude(X, y, sfm, handle)
        capi.check(capi.lib().nfm_opt_set_it(self._h, self.it))
        need = B * inner
        chunks = _IndexStream(n, need, self.shuffle, globalRand(), stream)
        if self.verbose > 0:
            print("Minibatch size: %d" % B)
            print("Number of inner iteration: %d" % inner)
            _echo_header(self.maxIter, viol=False)
        oldLossVal = float("inf")
        isConverged = False
        self.history = []
        for it in range(self.maxIter):
            ls, _ = self._epoch(X, chunks.chunk(it), 0, need)
            self.it += inner
            runningLoss = ls / float(B * inner)  # :122
            self.history.append((0.0, runningLoss))
            if callback is not None:  # :185-187
                self._finalize_into(sfm)
                callback(self, sfm)
            if math.isnan(runningLoss):  # :189-191
                print("Loss is NaN. Use smaller learning rate.")
                break
            if self.verbose > 0:  # :193-199
                self._finalize_into(sfm)
                regVal = _reg_penalty(self.reg, self.gamma, sfm, _l2_penalty(sfm, self.alpha0, self.alpha, self.beta))
                _echo_info(it + 1, self.maxIter, None, runningLoss, regVal)
            if abs(oldLossVal - runningLoss) < self.tol:  # :201-204
                if self.verbose > 0:
                    print("Converged at epoch %d." % (it + 1))
                isConverged = True
                break
            oldLossVal = runningLoss
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        self._finalize_into(sfm)
        return self


def predictAllWithGrad(X, y, sfm, loss="squared", lossParam=1.0):
    """optimizer/pgd.nim:70-103 on the device: -> (yPred, dL, grads) with grads = {"P": [nOrders][d+a][k] (the training
    layout of the reference's grads.P), "w": [d], "intercept": float, "loss": mean loss} -- the gradient of the mean
    loss at sfm's current parameters (sfm must be initialised; classification targets are sign()-ed)."""
    sfm.checkInitialized()

    def handle():
        # the device optimizer (and with it the one-batch plan of X, nfm_opt_predict_all_with_grad) is kept on the model:
        # PGD-style solvers ask for the full gradient of the same data once per iteration
        opt = getattr(sfm, "_grad_opt", None)
        if opt is None or opt._grad_key != (loss, float(lossParam)):
            opt = MBPSGD(maxIter=1, loss=loss, reg=newL1(), miniBatchSize=1, verbose=0, lossParam=lossParam)
            opt._grad_key = (loss, float(lossParam))
            sfm._grad_opt = opt
        opt._handle(sfm, X.ctx, "minibatch")
        return opt

    y, opt = _fit_prelude(X, y, sfm, handle)
    n, d = X.nSamples, X.nFeatures
    nb, k, da = sfm._P.shape
    yp, dL = np.zeros(n), np.zeros(n)
    gP, gw = np.zeros((nb, da, k)), np.zeros(d)
    gb, ls = C.c_double(0.0), C.c_double(0.0)
    capi.check(capi.lib().nfm_opt_predict_all_with_grad(opt._h, X.h, _vp(yp), _vp(dL), _vp(gP), _vp(gw), C.byref(gb),
                                                        C.byref(ls)))
    return yp, dL, {"P": gP, "w": gw, "intercept": gb.value, "loss": ls.value / max(n, 1)}


def newMBPSGD(maxIter=100, eta0=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None,
              miniBatchSize=-1, maxIterInner=-1, scheduling="optimal", power=1.0, verbose=1, tol=1e-6, shuffle=True,
              nCalls=-1, **gpu):
    return MBPSGD(maxIter, eta0, alpha0, alpha, beta, gamma, loss, reg, miniBatchSize, maxIterInner, scheduling, power,
                  verbose, tol, shuffle, nCalls, **gpu)


# ------------------------------------------------------------------------------------------------
# PSGD (optimizer/psgd.nim): SGD in the reference's sample order with the lazily updated L1 / L21
# ------------------------------------------------------------------------------------------------
_PSGD_SQUARED_MSG = ("PSGD on the device takes newL1() or newL21(): the step of %s touches every parameter per sample -- use "
                     "newMBPSGD(reg=%s), which has its proximal operator")


def _psgd_check_reg(reg):
    """which regularisers the device's PSGD has the lazy hooks for (psgd_seq.hip)"""
    if isinstance(reg, (SquaredL12, SquaredL21)):
        ctor = "new" + type(reg).__name__ + "()"
        raise ValueError(_PSGD_SQUARED_MSG % (type(reg).__name__, ctor))
    if isinstance(reg, (OmegaTI, OmegaCS)):
        raise ValueError("PSGD cannot be used for %s: it has no SGD hooks -- use %s" % (
            type(reg).__name__, "newPCD(reg=newOmegaTI())" if isinstance(reg, OmegaTI) else "newPBCD(reg=newOmegaCS())"))
    if not isinstance(reg, (L1, L21)):
        raise ValueError("reg must be newL1() or newL21()")


class PSGD(_OptimizerBase):
    """optimizer/psgd.nim:11-55,76-215: newPSGD(...).fit(X, y, sfm).  The per-sample step with the regulariser's lazy hooks,
    the cache resets and finalize run on the device (nfm_psgd_create / nfm_psgd_begin_fit / nfm_opt_epoch /
    nfm_psgd_finalize); the epoch loop, the sample order (Nim's global generator, or explicit perms), the nCalls split, the
    callbacks, the stopping rule (:198-201) and the verbose lines run here where the reference has them.

    reg: newL1() or newL21().  The reference's default is newSquaredL12() and so is this constructor's -- but the device has
    no PSGD step for SquaredL12 / SquaredL21 (it touches every parameter per sample), so A DEFAULT-CONSTRUCTED newPSGD() IS
    REFUSED AT fit with a ValueError that names newMBPSGD; pass reg=newL1() or reg=newL21()."""

    def __init__(self, maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None,
                 scheduling="optimal", power=1.0, verbose=1, tol=1e-3, shuffle=True, nCalls=-1, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, shuffle, nCalls, "sequential", 1, lossParam)
        if scheduling not in capi.SCHED:
            raise ValueError("unknown scheduling %r" % (scheduling,))
        self.reg = reg if reg is not None else newSquaredL12()  # psgd.nim:25
        if not isinstance(self.reg, _Regularizer):
            raise ValueError("reg must be a regularizer (newL1(), newL21(), ...)")
        self.gamma, self.eta0, self.scheduling, self.power = float(gamma), float(eta0), scheduling, float(power)

    def _create(self, mh, mode):
        cfg = capi.MBPSGDCfg(self.eta0, self.alpha0, self.alpha, self.beta, self.gamma, self.power, self.lossParam,
                             capi.LOSS[self.loss], capi.SCHED[self.scheduling], capi.REG[self.reg.name], 0, 1)
        capi.check(capi.lib().nfm_psgd_create(mh, C.byref(cfg), C.byref(self._h)))

    def _cfg_key(self):
        return super()._cfg_key() + (self.eta0, self.gamma, self.scheduling, self.power, self.reg.name)

    def setDataParallel(self, group, syncPeriod=0, overlap=True, combine="auto"):
        if group is not None:
            raise ValueError("PSGD has no data-parallel mode: one sample is in flight (newSGD / newAdaGrad in mini-batch mode have one)")

    def _finalize_into(self, sfm):
        capi.check(capi.lib().nfm_psgd_finalize(self._h))
        sfm._pull()

    def fit(self, X, y, sfm, callback=None, perms=None, devices=None):
        """perms ([maxIter][n], optional) replaces the internal shuffle with explicit permutations, as SGD.fit takes them."""
        _refuse_convex(sfm, "PSGD")
        _psgd_check_reg(self.reg)
        if not isinstance(sfm, FactorizationMachine):
            raise ValueError("PSGD fits a FactorizationMachine (psgd.nim:76-78): use newSGD or newAdaGrad for a field-aware model")
        if sfm.nComponents > 128:
            raise ValueError("PSGD on the device supports nComponents <= 128: use newMBPSGD(reg=newL1()) or newSGD for wider models")
        if sfm.degree > 6:
            raise ValueError("PSGD on the device supports degree <= 6: use newSGD(mode='sequential') beyond")
        if isinstance(X, StreamCSRDataset):
            raise ValueError("PSGD needs a resident dataset (its lazy caches follow one sample order), not a StreamCSRDataset: "
                             "use newSGD, which streams")
        if devices is not None:
            raise ValueError("PSGD runs on one device (one sample in flight): fit(devices=[...]) is for newSGD / newAdaGrad in mini-batch mode")
        sfm.init(X)
        y, _ = _fit_prelude(X, y, sfm, lambda: self._restart_handle(sfm, X.ctx, "sequential"))  # :106-107
        n = X.nSamples
        lib = capi.lib()
        capi.check(lib.nfm_opt_set_it(self._h, self.it))
        capi.check(lib.nfm_psgd_begin_fit(self._h, X.h))  # reg.initSGD, :112: the caches start afresh in every fit
        if self.verbose > 0:
            _echo_header(self.maxIter, viol=False)
        rng = globalRand()
        indices = np.arange(n, dtype=np.int64)
        if perms is not None:
            perms = [_i64(p_) for p_ in perms]
        isConverged = False
        runningLossOld = 0.0
        self.history = []
        self.lossSums = []  # the running loss of every epoch before :186 divides it
        for epoch in range(self.maxIter):
            runningLoss = 0.0
            perm = None
            if perms is not None:
                perm = perms[epoch]
            elif self.shuffle:
                rng.shuffle(indices)  # :120 (Nim's global generator there)
                perm = indices
            if callback is not None and self.nCalls > 0:  # :179-182
                runningLoss, _ = self._epoch_in_calls(X, perm, sfm, callback)
            else:
                runningLoss, _ = self._epoch(X, perm, 0, n)
                self.it += n
            self.lossSums.append(runningLoss)
            runningLoss /= float(n)  # :186
            self.history.append((0.0, runningLoss))
            if callback is not None and self.nCalls <= 0:  # :190-192
                self._finalize_into(sfm)
                callback(self, sfm)
            if math.isnan(runningLoss):  # :194-196
                print("Loss is NaN. Use smaller learning rate.")
                break
            if abs(runningLoss - runningLossOld) < self.tol:  # :198-201
                if self.verbose > 0:
                    print("Converged at epoch %d." % epoch)
                isConverged = True
                break
            if self.verbose > 0:  # :203-207: on the working values, not caught up
                sfm._pull()
                regVal = _reg_penalty(self.reg, self.gamma, sfm, _l2_penalty(sfm, self.alpha0, self.alpha, self.beta))
                _echo_info(epoch + 1, self.maxIter, None, runningLoss, regVal)
            runningLossOld = runningLoss
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        self._finalize_into(sfm)  # :215
        return self


def newPSGD(maxIter=100, eta0=0.01, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, scheduling="optimal",
            power=1.0, verbose=1, tol=1e-3, shuffle=True, nCalls=-1, **gpu):
    """psgd.nim:23-55.  reg defaults to newSquaredL12() as in the reference, which the device's PSGD refuses at fit: pass
    newL1() or newL21() (class PSGD)."""
    return PSGD(maxIter, eta0, alpha0, alpha, beta, gamma, loss, reg, scheduling, power, verbose, tol, shuffle, nCalls, **gpu)


# ------------------------------------------------------------------------------------------------
# full-batch proximal gradient: PGD, FISTA, NMAPGD (optimizer/pgd.nim, fista.nim, nmapgd.nim)
# ------------------------------------------------------------------------------------------------
class _PGDBase(_WholeIterSolver):
    """newPGD / newFISTA / newNMAPGD.  The algorithm -- gradient, line search, the accept / restart and Z / V branches -- runs
    in the library with every parameter set resident on the device (nfm_pgd_create / nfm_pgd_begin_fit / nfm_opt_epoch,
    DESIGN.md section 15); the stopping test is on the SQUARED distance, and the callback comes before the verbose line
    (pgd.nim:197-199).  history: (viol, lossVal, regVal) per iteration."""
    _algo = None
    _epoch_label_offset = 1  # the "Converged at epoch" line: pgd.nim:209 prints `epoch`, fista.nim:133 / nmapgd.nim:261 `it+1`

    def __init__(self, maxIter, alpha0, alpha, beta, gamma, loss, reg, rho, sigma, maxSearch, verbose, tol, lossParam, eta=0.5):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)
        self.gamma = float(gamma)
        self.reg = _matrix_prox_reg(reg)
        self.rho, self.sigma, self.maxSearch, self.eta = float(rho), float(sigma), int(maxSearch), float(eta)
        self.iterations = []  # nfm_pgd_last_iter of every iteration, as dicts

    def _params(self):
        return (self._algo, self.alpha0, self.alpha, self.beta, self.gamma, self.loss, self.lossParam, self.reg.name,
                self.reg.transpose, self.rho, self.sigma, self.maxSearch, self.eta)

    def _create(self, mh, out):
        return capi.lib().nfm_pgd_create(mh, capi.PGD_ALGO[self._algo], self.alpha0, self.alpha, self.beta, self.gamma, self.rho,
                                         self.sigma, self.eta, capi.LOSS[self.loss], self.lossParam, capi.REG[self.reg.name],
                                         int(self.reg.transpose), self.maxSearch, out)

    def _begin_fit(self, h, X, sfm):
        return capi.lib().nfm_pgd_begin_fit(h, X.h, int(bool(sfm.warmStart)))

    def _reset_records(self):
        self.history, self.iterations = [], []

    def last_iter(self):
        """nfm_pgd_last_iter as a dict"""
        out = (C.c_double * capi.PGD_IT_COUNT)()
        capi.check(capi.lib().nfm_pgd_last_iter(self._h, out))
        return {"lossVal": out[0], "regVal": out[1], "viol": out[2], "eta": (out[3], out[4]), "trials": (int(out[5]), int(out[6])),
                "branch": capi.PGD_BRANCH[int(out[7])], "t": out[8], "c": out[9], "q": out[10], "start": (out[11], out[12])}

    def _iteration(self, ls, vs, n):
        rec = self.last_iter()
        self.iterations.append(rec)
        self.history.append((rec["viol"], rec["lossVal"], rec["regVal"]))
        return rec["viol"], rec["lossVal"]

    def _reg_value(self, sfm, n):
        return self.history[-1][2]  # the library's own figure: nothing is pulled for the verbose line

    def _converged_label(self, it):
        return "epoch %d" % (it + self._epoch_label_offset)


class PGD(_PGDBase):
    """optimizer/pgd.nim:10-42,149-217"""
    _algo, _name = "pgd", "PGD"
    _epoch_label_offset = 0  # pgd.nim:209 prints `epoch`, not `epoch+1` (kept)


class FISTA(_PGDBase):
    """optimizer/fista.nim:10-43,52-141; t is kept on the optimizer for a warm-started model"""
    _algo, _name = "fista", "FISTA"


class NMAPGD(_PGDBase):
    """optimizer/nmapgd.nim:10-46,174-268; t, c, q and the caches are kept on the optimizer for a warm-started model.
    alpha0 is accepted and ignored: newNMAPGD stores alpha0: alpha (nmapgd.nim:44)."""
    _algo, _name = "nmapgd", "NMAPGD"


def newPGD(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, rho=0.5, sigma=1.0,
           maxSearch=-1, verbose=1, tol=1e-6, lossParam=1.0):
    """optimizer/pgd.nim:19-42; reg=None is newSquaredL12() (column-wise), the reference's default"""
    return PGD(maxIter, alpha0, alpha, beta, gamma, loss, reg, rho, sigma, maxSearch, verbose, tol, lossParam)


def newFISTA(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, rho=0.5, sigma=1.0,
             maxSearch=-1, verbose=1, tol=1e-6, lossParam=1.0):
    """optimizer/fista.nim:20-43"""
    return FISTA(maxIter, alpha0, alpha, beta, gamma, loss, reg, rho, sigma, maxSearch, verbose, tol, lossParam)


def newNMAPGD(maxIter=100, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, rho=0.5, sigma=0.01,
              maxSearch=-1, eta=0.50, verbose=1, tol=1e-5, lossParam=1.0):
    """optimizer/nmapgd.nim:20-46"""
    return NMAPGD(maxIter, alpha0, alpha, beta, gamma, loss, reg, rho, sigma, maxSearch, verbose, tol, lossParam, eta)


# ------------------------------------------------------------------------------------------------
# Katyusha (optimizer/katyusha.nim)
# ------------------------------------------------------------------------------------------------
class Katyusha(_WholeIterSolver):
    """optimizer/katyusha.nim:11-53,156-269: newKatyusha(...).fit(X, y, sfm).  The seven parameter sets, the variance-reduced
    mini-batch gradient and the dense updates of the inner loop stay on the device (nfm_katyusha_create /
    nfm_katyusha_begin_fit / nfm_opt_epoch); one nfm_opt_epoch call is one outer iteration.  The index
    stream (indices[ii] with wrap-around and reshuffle, :108-118), the stopping rule on viol, the verbose lines and the
    per-epoch callback run here where the reference has them.  After every outer iteration sfm holds what finalize (:56-73)
    gives the user.  Nothing is carried between fits.  history: (viol, lossVal) per outer iteration.

    Departures: beta <= 0, alpha <= 0 with fitLinear, alpha0 <= 0 with fitIntercept and eta <= 0 are
    ValueError (the reference returns NaN parameters: (1 - theta) / (1 - theta^m) is 0 / 0); nCalls > 0 is refused."""
    _name = "Katyusha"
    _nan_stops = True  # :245-247

    def __init__(self, maxIter=100, eta=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None,
                 miniBatchSize=-1, tau1=0.5, tau2=-1.0, verbose=1, tol=1e-6, shuffle=True, nCalls=-1, lossParam=1.0):
        super().__init__(maxIter, alpha0, alpha, beta, loss, verbose, tol, lossParam)
        self.reg = _matrix_prox_reg(reg)
        if int(nCalls) > 0:
            raise ValueError("Katyusha: nCalls > 0 (a callback inside the inner loop) is not supported; nCalls <= 0 calls the "
                             "callback once per epoch")
        self.eta, self.gamma, self.tau1, self.tau2 = float(eta), float(gamma), float(tau1), float(tau2)
        self.miniBatchSize, self.shuffle, self.nCalls = int(miniBatchSize), bool(shuffle), int(nCalls)
        self.batch = None  # the mini-batch size of the last fit
        if not self.eta > 0.0:
            raise ValueError("eta must be > 0")
        if not self.beta > 0.0:
            raise ValueError("beta must be > 0: the scale of next_tilde, (1 - theta) / (1 - theta^m), is 0 / 0 otherwise")

    def _params(self):
        return (self.eta, self.alpha0, self.alpha, self.beta, self.gamma, self.tau1, self.tau2, self.loss, self.lossParam,
                self.reg.name, self.reg.transpose, self.batch)

    def _create(self, mh, out):
        return capi.lib().nfm_katyusha_create(mh, self.eta, self.alpha0, self.alpha, self.beta, self.gamma, self.tau1, self.tau2,
                                              capi.LOSS[self.loss], self.lossParam, capi.REG[self.reg.name],
                                              int(self.reg.transpose), self.batch, out)

    def _begin_fit(self, h, X, sfm):
        return capi.lib().nfm_katyusha_begin_fit(h, X.h)

    def _check(self, sfm):
        if sfm.fitLinear and not self.alpha > 0.0:
            raise ValueError("alpha must be > 0 with fitLinear: the scale of next_tilde, (1 - theta) / (1 - theta^m), is 0 / 0 otherwise")
        if sfm.fitIntercept and not self.alpha0 > 0.0:
            raise ValueError("alpha0 must be > 0 with fitIntercept: the scale of next_tilde, (1 - theta) / (1 - theta^m), is 0 / 0 otherwise")

    def _resolve(self, X, sfm):
        self.batch = self.miniBatchSize if self.miniBatchSize > 0 else _default_batch(X)  # :203-206
        _check_degree2(self.reg, sfm)

    def _chunks(self, X, stream):
        inner = (X.nSamples - 1) // self.batch + 1  # :207
        need = self.batch * inner
        chunks = _IndexStream(X.nSamples, need, self.shuffle, globalRand(), stream)
        if self.verbose > 0:
            print("Minibatch size: %d" % self.batch)
            print("Number of inner iteration: %d" % inner)
        return lambda it: (chunks.chunk(it), 0, need)

    def snapshot(self, sfm):
        """tilde_params (the snapshot the verbose line's regVal is taken on) -> (P [nOrders][d+a][k], w, intercept)"""
        nb, k, da = sfm._P.shape
        P, w, b = np.zeros((nb, da, k)), np.zeros(len(sfm._w)), C.c_double(0.0)
        capi.check(capi.lib().nfm_katyusha_snapshot(self._h, _vp(P), _vp(w), C.byref(b)))
        return P, w, b.value

    def _reg_value(self, sfm, n):
        """:249-253: regVal on tilde.  snapshot gives every order as reg.eval takes it, [d+a][k]"""
        tP, tw, tb = self.snapshot(sfm)
        regVal = _l2_penalty(SimpleNamespace(P=tP, w=tw, intercept=tb), self.alpha0, self.alpha, self.beta)
        for order in range(tP.shape[0]):
            regVal += self.gamma * self.reg.eval(tP[order], sfm.degree - order)
        return regVal

    def _converged_label(self, it):
        return "epoch %d" % (it + 1)

    def fit(self, X, y, sfm, callback=None, stream=None):
        """katyusha.nim:156-269.  stream (optional): the sample indices in the order the inner loops consume them, at least
        maxIter * miniBatchSize * maxIterInner of them -- replaces the internal shuffle, as for MBPSGD.fit.  The loss of a
        history entry is the one at the snapshot the epoch started from (:241-244); the callback sees finalize's model."""
        return self._fit(X, y, sfm, callback, stream)


def newKatyusha(maxIter=100, eta=0.1, alpha0=1e-6, alpha=1e-3, beta=1e-4, gamma=1e-4, loss="squared", reg=None, miniBatchSize=-1,
                tau1=0.5, tau2=-1.0, verbose=1, tol=1e-6, shuffle=True, nCalls=-1, lossParam=1.0):
    """optimizer/katyusha.nim:24-53; reg=None is newSquaredL12() (column-wise), the reference's default"""
    return Katyusha(maxIter, eta, alpha0, alpha, beta, gamma, loss, reg, miniBatchSize, tau1, tau2, verbose, tol, shuffle, nCalls,
                    lossParam)


# ------------------------------------------------------------------------------------------------
# Hazan's algorithm for the convex factorization machine (optimizer/hazan.nim)
# ------------------------------------------------------------------------------------------------
class _ConvexSolver(_OptHandle):
    """What Hazan and GreedyCD share: a resident ConvexFactorizationMachine and the power method's start vector.  Subclass: _name, _params, _create."""
    _name = None

    def _refuse(self, X, cfm):
        if not isinstance(cfm, ConvexFactorizationMachine):
            raise ValueError("%s fits a ConvexFactorizationMachine" % self._name)
        if isinstance(X, StreamCSRDataset):
            raise ValueError("%s needs a resident dataset (the reference's fit takes a ColDataset)" % self._name)

    def _begin(self, X, y, cfm):  # init, the targets and the device optimizer -> its handle
        cfm.init(X)
        return _fit_prelude(X, y, cfm, lambda: self._handle(cfm, X.ctx), colWise=True)[1]

    @staticmethod
    def _start_vector(d, powerInit):
        """powerInit(d), or the d draws of 2*rand(1.0) - 1.0 from the global generator (tensor.nim:920-921)"""
        start = _f64(powerInit(d)) if powerInit is not None else 2 * globalRand().rand(d, 1.0) - 1.0
        if start.shape != (d,):
            raise ValueError("powerInit must return nFeatures values")
        return start


class Hazan(_ConvexSolver):
    """optimizer/hazan.nim:8-46,59-225: newHazan(...).fit(X, y, cfm).  The reference fits a ColDataset; the library builds the
    column twin of the row dataset itself.  yPredLinear, yPredQuad, the residual, K, P, lams, w, colNormSq and the vectors of
    the power method and of CG stay on the device for the whole fit (nfm_hazan_create / nfm_hazan_begin_fit / nfm_hazan_iter,
    DESIGN.md section 20); per outer iteration one record comes back.  The outer loop, the nTol stopping rule, the verbose line
    and the callback run here where the reference has them, and so does the draw of the power method's start vector from
    Nim's global generator.  Squared loss only; alpha0 / alpha / beta of the model family are ignored (:10-13).
    history: one dict per outer iteration (capi.HAZAN_REC: loss, trace, slot, step, powerIters, cgIters, eval, nComponents).
    self.it persists across warm-started fits and is not incremented on the converging iteration (:211-222).

    The one deviation: the reference's cg cannot leave on its iteration cap (tensor.nim:992 never increments `it`) and spins
    on a zero right-hand side; here it ends after 1000 iterations and when curv is 0 or not finite."""
    _name = "Hazan"

    def __init__(self, maxIter=100, eta=1000.0, verbose=2, tol=1e-7, nTol=10, maxIterPower=1000, tolPower=1e-7, optimal=True):
        self.maxIter, self.eta, self.verbose, self.tol = int(maxIter), float(eta), int(verbose), float(tol)
        self.nTol, self.maxIterPower, self.tolPower, self.optimal = int(nTol), int(maxIterPower), float(tolPower), bool(optimal)
        self.it = 0
        self.history = []

    def _params(self):
        return (self.eta, self.maxIterPower, self.tolPower, self.optimal)

    def _create(self, mh, out):
        return capi.lib().nfm_hazan_create(mh, self.eta, self.maxIterPower, self.tolPower, int(self.optimal), out)

    def fit(self, X, y, cfm, callback=None, powerInit=None):
        """hazan.nim:59-225.  powerInit (optional): callable(nFeatures) -> the power method's start vector of one outer
        iteration, in place of the d draws of 2*rand(1.0) - 1.0 from the global generator (tensor.nim:920-921)."""
        self._refuse(X, cfm)
        h = self._begin(X, y, cfm)
        lossOld = C.c_double(0.0)
        capi.check(capi.lib().nfm_hazan_begin_fit(h, X.h, C.byref(lossOld)))
        lossOld = lossOld.value
        if not cfm.warmStart:
            self.it = 0  # :87-88
        d = X.nFeatures
        nc = cfm.nComponents
        self.history = []
        nTol, isConverged = 0, False
        rec = (C.c_double * len(capi.HAZAN_REC))()
        for _ in range(self.maxIter):
            if not self.optimal and nc >= cfm.maxComponents:  # :137-138
                break
            start = self._start_vector(d, powerInit)
            capi.check(capi.lib().nfm_hazan_iter(h, X.h, self.it, _vp(start), rec))
            r = dict(zip(capi.HAZAN_REC, rec))
            for key in ("slot", "powerIters", "cgIters", "nComponents"):
                r[key] = int(r[key])
            self.history.append(r)
            nc = r["nComponents"]
            if callback is not None:  # :198-199
                cfm._pull()
                callback(self, cfm)
            lossNew = r["loss"]
            if self.verbose > 0:  # :203-209
                print("Epoch: %s   MSE/2: %1.4e   Trace Norm: %1.4e" % (str(self.it).rjust(len(str(self.maxIter))), lossNew / 2.0,
                                                                        r["trace"]), flush=True)
            if lossOld - lossNew < self.tol:  # :211-219
                nTol += 1
                if nTol >= self.nTol:
                    if self.verbose > 0:
                        print("Converged at iteration %d." % (self.it + 1))
                    isConverged = True
                    break
            else:
                nTol = 0
            lossOld = lossNew
            self.it += 1
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        cfm._pull()
        return self


def newHazan(maxIter=100, eta=1000.0, verbose=2, tol=1e-7, nTol=10, maxIterPower=1000, tolPower=1e-7, optimal=True):
    """optimizer/hazan.nim:22-46"""
    return Hazan(maxIter, eta, verbose, tol, nTol, maxIterPower, tolPower, optimal)


# ------------------------------------------------------------------------------------------------
# Greedy coordinate descent for the convex factorization machine (optimizer/greedy_cd.nim)
# ------------------------------------------------------------------------------------------------
class GreedyCD(_ConvexSolver):
    """optimizer/greedy_cd.nim:8-66,76-109,320-500 at refitFully = false: newGreedyCD(...).fit(X, y, cfm), the default solver of the
    reference's nimfm_cfm.  yPred, dL, K, P, lams, w, colNormSq and the power method's vectors stay on the device for the whole
    fit (nfm_gcd_*); per step one record comes back.  The outer and the inner loop, both stopping tests,
    the refit schedule, the verbose lines and the callback run here where the reference has them, and so does the draw of the
    power method's start vector from Nim's global generator -- only in the inner iterations that add a base, as the reference
    draws it.  All four losses; alpha0 / alpha / beta as the reference scales them.  A component thresholded to zero stays in
    the model (its slot is the next one used), so cfm.lams may hold zeros.  There is no self.it.
    history: one dict per outer iteration: loss, reg, nComponents (non-zero lams), objOld (fitZ's) and inner, the list of the
    inner iterations' records (capi.GCD_REC plus it, refit, checked).
    refitFully = true (ADMM, Newton-CG, two dsyev calls) stays with the reference: fit raises ValueError.  sigma, maxIterADMM,
    tolADMM and maxIterLineSearch belong to it: accepted and unused."""
    _name = "GreedyCD"

    def __init__(self, maxIter=10, alpha0=1e-6, alpha=1e-3, beta=1e-5, loss="squared", maxIterInner=10, nRefitting=10, refitFully=False,
                 verbose=1, tol=1e-7, maxIterPower=100, tolPower=1e-7, sigma=1e-4, maxIterADMM=100, tolADMM=1e-4, maxIterLineSearch=100,
                 lossParam=1.0):
        if loss not in capi.LOSS:
            raise ValueError("unknown loss %r" % (loss,))
        if int(nRefitting) < 1:
            raise ValueError("nRefitting < 1.")  # the reference would divide by zero (greedy_cd.nim:384)
        self.maxIter, self.alpha0, self.alpha, self.beta = int(maxIter), float(alpha0), float(alpha), float(beta)
        self.loss, self.lossParam = loss, float(lossParam)
        self.maxIterInner, self.nRefitting, self.refitFully = int(maxIterInner), int(nRefitting), bool(refitFully)
        self.verbose, self.tol, self.maxIterPower, self.tolPower = int(verbose), float(tol), int(maxIterPower), float(tolPower)
        self.sigma, self.maxIterADMM, self.tolADMM, self.maxIterLineSearch = float(sigma), int(maxIterADMM), float(tolADMM), int(maxIterLineSearch)
        self.history = []

    def _params(self):
        return (self.alpha0, self.alpha, self.beta, self.loss, self.lossParam, self.maxIterPower, self.tolPower, self.refitFully)

    def _create(self, mh, out):
        return capi.lib().nfm_gcd_create(mh, self.alpha0, self.alpha, self.beta, capi.LOSS[self.loss], self.lossParam,
                                         self.maxIterPower, self.tolPower, int(self.refitFully), out)

    def fit(self, X, y, cfm, callback=None, powerInit=None):
        """greedy_cd.nim:415-500.  powerInit (optional): callable(nFeatures) -> the power method's start vector of one inner
        iteration that adds a base, in place of the d draws of 2*rand(1.0) - 1.0 from the global generator."""
        self._refuse(X, cfm)
        if int(self.nRefitting) < 1:
            raise ValueError("nRefitting < 1.")
        h = self._begin(X, y, cfm)
        L = capi.lib()
        lossOld, regOld = C.c_double(0.0), C.c_double(0.0)
        rc = L.nfm_gcd_begin_fit(h, X.h, C.byref(lossOld), C.byref(regOld))
        if rc == capi.ERR_UNSUPPORTED and self.refitFully:  # the reference raises nothing here: it runs ADMM with two dsyev calls
            raise ValueError(L.nfm_last_error().decode("utf-8", "replace"))
        capi.check(rc)
        lossOld, regOld = lossOld.value, regOld.value
        d, maxc = X.nFeatures, cfm.maxComponents
        self.history = []
        isConverged = False
        rec = (C.c_double * len(capi.GCD_REC))()
        for it in range(self.maxIter):
            if self.verbose > 0:
                print("Outer Iteration %d" % (it + 1))
            # fitInterceptCD, fitLinearCD and fitZ's head (:464-469, :332-336)
            capi.check(L.nfm_gcd_outer_begin(h, X.h, rec))
            nc, objOld = int(rec[5]), rec[6]
            outer = dict(nComponentsStart=nc, objOld=objOld, inner=[])
            for itIn in range(self.maxIterInner):  # fitZ (:347-412)
                start = self._start_vector(d, powerInit) if nc < maxc else None
                refit = (itIn + 1) % self.nRefitting == 0
                capi.check(L.nfm_gcd_inner(h, X.h, _vp(start), int(refit), rec))
                r = dict(zip(capi.GCD_REC, rec))
                for key in ("added", "slot", "powerIters", "nComponents", "nStored"):
                    r[key] = int(r[key])
                nc = r["nComponents"]
                r["it"], r["refit"] = itIn, refit
                r["checked"] = bool(r["added"]) or refit or itIn == self.maxIterInner - 1
                outer["inner"].append(r)
                if r["checked"]:  # :392-412
                    objNew = r["objective"]
                    if self.verbose > 1:
                        print("   Iteration: %s   Objective: %1.4e   Decreasing: %1.4e" % (str(itIn + 1).rjust(len(str(self.maxIterInner))),
                                                                                           objNew, objOld - objNew), flush=True)
                    if abs(objNew - objOld) < self.tol:
                        if self.verbose > 1:
                            print("   Converged at iteration %d." % (itIn + 1))
                        break
                    objOld = objNew
            lossNew, regNew = C.c_double(0.0), C.c_double(0.0)
            # the reference rebuilds yPred after the stopping test, when it goes on (:493-497); nothing reads yPred in between
            # but the test itself, so the rebuild is asked for here and is a no-op for the last iteration
            capi.check(L.nfm_gcd_outer_end(h, X.h, int(it < self.maxIter - 1), C.byref(lossNew), C.byref(regNew)))
            lossNew, regNew = lossNew.value, regNew.value
            outer.update(loss=lossNew, reg=regNew, nComponents=nc)
            self.history.append(outer)
            if callback is not None:  # :478-479
                cfm._pull()
                callback(self, cfm)
            if self.verbose > 0:
                print("   Loss: %1.4e   Reg: %1.4e" % (lossNew, regNew), flush=True)
            if abs(lossNew + regNew - lossOld - regOld) < self.tol:
                if self.verbose > 0:
                    print("Converged at iteration %d." % (it + 1))
                isConverged = True
                break
            lossOld, regOld = lossNew, regNew
        if not isConverged and self.verbose > 0:
            print("Objective did not converge. Increase maxIter.")
        cfm._pull()
        return self


def newGreedyCD(maxIter=10, alpha0=1e-6, alpha=1e-3, beta=1e-5, loss="squared", maxIterInner=10, nRefitting=10, refitFully=False,
                verbose=1, tol=1e-7, maxIterPower=100, tolPower=1e-7, sigma=1e-4, maxIterADMM=100, tolADMM=1e-4, maxIterLineSearch=100,
                lossParam=1.0):
    """optimizer/greedy_cd.nim:25-30 (lossParam: the Huber threshold, newHuber(threshold))"""
    return GreedyCD(maxIter, alpha0, alpha, beta, loss, maxIterInner, nRefitting, refitFully, verbose, tol, maxIterPower, tolPower, sigma,
                    maxIterADMM, tolADMM, maxIterLineSearch, lossParam)
