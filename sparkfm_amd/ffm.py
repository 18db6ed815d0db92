"""Field-aware factorization machines (include/fmhip_ffm.h): every feature keeps one factor vector per FIELD, and a pair of entries
interacts through the vectors each keeps for the other's field (Juan et al., RecSys 2016; libffm, xLearn).

    train = FFMDataSet.from_rows(rows, y, batch_rows=256)          # rows: lists of (field, feature, value)
    model = FFM(train, 4).learnWith(HipFFM.run(loss="logistic", optimizer="adagrad", eta=0.2, regv=2e-5, maxIteration=20))
    model.computeLogLoss(test), model.computeAUC(test)

A model and kernels of their own beside the FM path; there is no CPU fallback.  Scoring a prediction vector is host arithmetic."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel


class FFMDataSet:
    """Rows of (field, feature, value) entries with a label each, on the device: every row sorted by (field, feature), every
    mini-batch's transpose built once (fmhip_ffm_dataset_create)."""

    def __init__(self, row_ptr, col, field, val, y=None, batch_rows=0, normalize=False, device=0):
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        self.col = np.ascontiguousarray(col, np.int32)
        self.field = np.ascontiguousarray(field, np.int32)
        self.val = np.ascontiguousarray(val, np.float64).copy()
        self.y = None if y is None else np.ascontiguousarray(y, np.float64)
        n = len(self.row_ptr) - 1
        if n < 0 or not (len(self.col) == len(self.field) == len(self.val) == int(self.row_ptr[-1])):
            raise ValueError("row_ptr, col, field and val do not describe the same rows")
        if self.y is not None and self.y.shape != (n,):
            raise ValueError("y must hold one label per row (%d), not shape %r" % (n, self.y.shape))
        if normalize and len(self.val):          # libffm's instance-wise scaling: every row to unit L2 norm (an all-zero row stays)
            row_of = np.repeat(np.arange(n), np.diff(self.row_ptr))
            sq = np.bincount(row_of, self.val ** 2, minlength=n)
            self.val *= (1.0 / np.sqrt(np.where(sq > 0, sq, 1.0)))[row_of]
        self.size, self.batch_rows, self.device, self.normalized = n, int(batch_rows), int(device), bool(normalize)
        self._h = None

    @classmethod
    def from_arrays(cls, row_ptr, col, field, val, y=None, **kw):
        return cls(row_ptr, col, field, val, y, **kw)

    @classmethod
    def from_rows(cls, rows, y=None, num_fields=None, batch_rows=0, normalize=False, device=0):
        """rows: one list of (field, feature, value) per data row.  num_fields: when given, a field id outside [0, num_fields) raises."""
        ptr = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        flat = [e for r in rows for e in r]
        field = np.asarray([e[0] for e in flat], np.int32)
        if num_fields is not None and len(field) and (field.min() < 0 or field.max() >= num_fields):
            raise ValueError("a field id lies outside [0, %d)" % num_fields)
        return cls(ptr, np.asarray([e[1] for e in flat], np.int32), field, np.asarray([e[2] for e in flat], np.float64), y,
                   batch_rows=batch_rows, normalize=normalize, device=device)

    @property
    def handle(self):
        if self._h is None:
            h = C.c_void_p()
            _ffi.check(_ffi.load().fmhip_ffm_dataset_create(self.device, self.size, _ffi.ptr(self.row_ptr), _ffi.ptr(self.col), _ffi.ptr(self.field),
                                                           _ffi.ptr(self.val), _ffi.ptr(self.y), self.batch_rows, C.byref(h)))
            self._h = h
        return self._h

    def cache(self):
        self.handle
        return self

    def info(self):
        """dict of n_rows, nnz, dimension (largest feature id), fields (largest field id + 1), max_row, batch_rows, n_batches."""
        i64, i32 = C.c_int64, C.c_int32
        v = [i64(), i64(), i64(), i32(), i32(), i64(), i64()]
        _ffi.check(_ffi.load().fmhip_ffm_dataset_info(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("n_rows", "nnz", "dimension", "fields", "max_row", "batch_rows", "n_batches"), (x.value for x in v)))

    @property
    def n_batches(self):
        return self.info()["n_batches"]

    @property
    def dimension(self):
        return int(self.col.max()) if len(self.col) else 0

    @property
    def num_fields(self):
        return int(self.field.max()) + 1 if len(self.field) else 1

    def close(self):
        if self._h is not None:
            _ffi.load().fmhip_ffm_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FFMModel(FieldModel):
    """w0, w [n + 1] and v [n + 1, F, k] on the device (fmhip_ffm_model_t).  New parameters are zero; FFM.learnWith draws libffm's init."""

    _prefix = "fmhip_ffm"

    def __init__(self, num_attribute, num_fields, num_factor, device=0, stream=None):
        self._create(num_attribute, num_fields, num_factor, device, stream)

    def _shape(self):
        return (self.num_attribute + 1, self.num_fields, self.num_factor)

    def get_params(self):
        w0, w, v = C.c_double(), np.zeros(self.num_attribute + 1), np.zeros(self._shape())
        _ffi.check(_ffi.load().fmhip_ffm_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v)))
        return w0.value, w, v

    def set_params(self, w0, w, v):
        w, v = np.ascontiguousarray(w, np.float64), np.ascontiguousarray(v, np.float64)
        if w.shape != (self.num_attribute + 1,) or v.shape != self._shape():
            raise ValueError("w must have shape %r and v shape %r" % ((self.num_attribute + 1,), self._shape()))
        _ffi.check(_ffi.load().fmhip_ffm_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])

    def adagrad_state(self):
        """(n0, nw [n + 1], nv [n + 1, F, k]): AdaGrad's accumulators (a model under SGD raises)."""
        n0, nw, nv = C.c_double(), np.zeros(self.num_attribute + 1), np.zeros(self._shape())
        _ffi.check(_ffi.load().fmhip_ffm_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv)))
        return n0.value, nw, nv

    def set_adagrad_state(self, n0, nw, nv):
        nw, nv = np.ascontiguousarray(nw, np.float64), np.ascontiguousarray(nv, np.float64)
        if nw.shape != (self.num_attribute + 1,) or nv.shape != self._shape():
            raise ValueError("nw must have shape %r and nv shape %r" % ((self.num_attribute + 1,), self._shape()))
        _ffi.check(_ffi.load().fmhip_ffm_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv)))


class HipFFM(FieldLearner):
    """The FFM learner: mini-batch SGD or AdaGrad with libffm's lazy regularisation (only what a batch touches moves).
    linear=False is libffm's model: w0 and w are left as they are (0 from FFM.learnWith) and never stepped."""

    _prefix = "fmhip_ffm"          # (no array of its own: no _flag, three regularisers)

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.2, regv=2e-5, regw=0.0, reg0=0.0, linear=True, maxIteration=10, seed=0,
                 adagrad_eps=1e-10, adagrad_init=1.0):
        self.loss_code, self.opt_code = _ffi.loss_code(loss), _ffi.optimizer_code(optimizer)
        self.adagrad_eps, self.adagrad_init = _ffi.adagrad_settings(adagrad_eps, adagrad_init)
        for name, x in (("eta", eta), ("regv", regv), ("regw", regw), ("reg0", reg0)):
            if not (np.isfinite(x) and x >= 0):
                raise ValueError("%s must be finite and >= 0, not %r" % (name, x))
        if not isinstance(linear, bool):
            raise ValueError("linear must be True or False, not %r" % (linear,))
        self.loss, self.optimizer, self.linear = loss, optimizer, linear
        self.eta, self.regv, self.regw, self.reg0 = float(eta), float(regv), float(regw), float(reg0)
        self.rates = (self.reg0, self.regw, self.regv)
        self.maxIteration, self.seed = int(maxIteration), int(seed)
        self.last_stats = None


def libffm_init(seed, num_attribute, num_fields, num_factor):
    """libffm's initial factors: V ~ U[0, 1) / sqrt(k), drawn on the host from `seed`, shape (n + 1, F, k)."""
    return np.random.default_rng(seed).random((num_attribute + 1, num_fields, num_factor)) / np.sqrt(num_factor)


class FFM:
    """FFM(train, k).learnWith(HipFFM.run(...)) -> FFMModel, as FM(train, k).learnWith(...) gives an FMModel."""

    def __init__(self, dataset, num_factor, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor = dataset, int(num_factor)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = FFMModel(self.num_attribute, self.num_fields, self.num_factor, device=self.dataset.device)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), libffm_init(learner.seed, self.num_attribute, self.num_fields, self.num_factor))
        return learner.fit(model, self.dataset)
