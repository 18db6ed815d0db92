"""Field-weighted factorization machines (include/fmhip_fwfm.h): one factor vector per feature, as the plain FM keeps, and one learned
weight r[f][g] per pair of FIELDS (Pan et al., WWW 2018) — the field-pair strengths of the FFM without its F vectors per feature.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = FwFM(train, 16).learnWith(HipFwFM.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.r

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel


class FwFMModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k] and the symmetric r [F, F] on the device (fmhip_fwfm_model_t).  A new model has v = w = w0 = 0 and
    r = 1; FwFM.learnWith draws v."""

    _prefix = "fmhip_fwfm"

    def __init__(self, num_attribute, num_fields, num_factor, device=0, stream=None):
        self._create(num_attribute, num_fields, num_factor, device, stream)

    def _zeros(self):
        return np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)), np.zeros((self.num_fields, self.num_fields))

    def _checked(self, names, arrays):
        out = [np.ascontiguousarray(x, np.float64) for x in arrays]
        for name, x, like in zip(names, out, self._zeros()):
            if x.shape != like.shape:
                raise ValueError("%s must have shape %r, not %r" % (name, like.shape, x.shape))
        return out

    def get_params(self):
        """(w0, w, v, r)."""
        w0, (w, v, r) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_fwfm_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _ffi.ptr(r)))
        return w0.value, w, v, r

    def set_params(self, w0, w, v, r):
        w, v, r = self._checked("wvr", (w, v, r))
        _ffi.check(_ffi.load().fmhip_fwfm_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _ffi.ptr(r)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    r = property(lambda self: self.get_params()[3])

    def adagrad_state(self):
        """(n0, nw [n + 1], nv [n + 1, k], nr [F, F]): AdaGrad's accumulators (a model under SGD raises)."""
        n0, (nw, nv, nr) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_fwfm_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _ffi.ptr(nr)))
        return n0.value, nw, nv, nr

    def set_adagrad_state(self, n0, nw, nv, nr):
        nw, nv, nr = self._checked(("nw", "nv", "nr"), (nw, nv, nr))
        _ffi.check(_ffi.load().fmhip_fwfm_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _ffi.ptr(nr)))


class HipFwFM(FieldLearner):
    """The FwFM learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, r and w0 every batch.
    field_weights=False never steps r (with r = 1: the plain FM); linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_fwfm", "field_weights", "regr"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regr=0.0, linear=True, field_weights=True,
                 maxIteration=10, seed=0, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regr, linear, field_weights, maxIteration, adagrad_eps, adagrad_init)
        self.seed = int(seed)


def fwfm_init(seed, num_attribute, num_factor):
    """The initial factors: v ~ U[0, 1) / sqrt(k), drawn on the host from `seed`, shape (n + 1, k) (libffm's draw, one vector a feature)."""
    return np.random.default_rng(seed).random((num_attribute + 1, num_factor)) / np.sqrt(num_factor)


class FwFM:
    """FwFM(train, k).learnWith(HipFwFM.run(...)) -> FwFMModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor = dataset, int(num_factor)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = FwFMModel(self.num_attribute, self.num_fields, self.num_factor, device=self.dataset.device)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), fwfm_init(learner.seed, self.num_attribute, self.num_factor),
                         np.ones((self.num_fields, self.num_fields)))
        return learner.fit(model, self.dataset)
