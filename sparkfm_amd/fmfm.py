"""Field-matrixed factorization machines, FmFM / FM^2 (include/fmhip_fmfm.h): one factor vector per feature, as the plain FM keeps, and
one learned k x k matrix M[f][g] per pair of FIELDS (Sun et al., WWW 2021) — between the FwFM's scalar per pair and the FFM's F vectors
per feature.  Entries of one field are sum-pooled; M[g][f] is M[f][g] transposed and M[f][f] is 0.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = FmFM(train, 16).learnWith(HipFmFM.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.m

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel


def identity_matrices(num_fields, num_factor):
    """M of a new model, (F, F, k, k): I for every pair f != g, 0 on the diagonal blocks."""
    m = np.zeros((num_fields, num_fields, num_factor, num_factor))
    m[:] = np.eye(num_factor)
    m[np.arange(num_fields), np.arange(num_fields)] = 0.0
    return m


class FmFMModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k] and the field matrices m [F, F, k, k] on the device (fmhip_fmfm_model_t).  A new model has
    v = w = w0 = 0 and m[f][g] = I for f != g; FmFM.learnWith draws v."""

    _prefix = "fmhip_fmfm"

    def __init__(self, num_attribute, num_fields, num_factor, device=0, stream=None):
        self._create(num_attribute, num_fields, num_factor, device, stream)

    def _zeros(self):
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                np.zeros((self.num_fields, self.num_fields, self.num_factor, self.num_factor)))

    def _checked(self, names, arrays):
        out = [np.ascontiguousarray(x, np.float64) for x in arrays]
        for name, x, like in zip(names, out, self._zeros()):
            if x.shape != like.shape:
                raise ValueError("%s must have shape %r, not %r" % (name, like.shape, x.shape))
        return out

    def get_params(self):
        """(w0, w, v, m)."""
        w0, (w, v, m) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_fmfm_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _ffi.ptr(m)))
        return w0.value, w, v, m

    def set_params(self, w0, w, v, m):
        w, v, m = self._checked("wvm", (w, v, m))
        _ffi.check(_ffi.load().fmhip_fmfm_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _ffi.ptr(m)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    m = property(lambda self: self.get_params()[3])

    def adagrad_state(self):
        """(n0, nw [n + 1], nv [n + 1, k], nm [F, F, k, k]): AdaGrad's accumulators (a model under SGD raises)."""
        n0, (nw, nv, nm) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_fmfm_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _ffi.ptr(nm)))
        return n0.value, nw, nv, nm

    def set_adagrad_state(self, n0, nw, nv, nm):
        nw, nv, nm = self._checked(("nw", "nv", "nm"), (nw, nv, nm))
        _ffi.check(_ffi.load().fmhip_fmfm_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _ffi.ptr(nm)))


class HipFmFM(FieldLearner):
    """The FmFM learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the field matrices and w0 every batch.
    field_matrices=False never steps m (with m = I: the plain FM on rows of one entry per field); linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_fmfm", "field_matrices", "regm"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regm=0.0, linear=True, field_matrices=True,
                 maxIteration=10, seed=0, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regm, linear, field_matrices, maxIteration, adagrad_eps, adagrad_init)
        self.seed = int(seed)


class FmFM:
    """FmFM(train, k).learnWith(HipFmFM.run(...)) -> FmFMModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor = dataset, int(num_factor)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        from .fwfm import fwfm_init          # the same draw: one vector a feature
        model = FmFMModel(self.num_attribute, self.num_fields, self.num_factor, device=self.dataset.device)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), fwfm_init(learner.seed, self.num_attribute, self.num_factor),
                         identity_matrices(self.num_fields, self.num_factor))
        return learner.fit(model, self.dataset)
