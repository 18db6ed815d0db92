"""Field-matrixed factorization machines, FmFM / FM^2 (include/fmhip_fmfm.h): one factor vector per feature, as the plain FM keeps, and
one learned k x k matrix M[f][g] per pair of FIELDS (Sun et al., WWW 2021) — between the FwFM's scalar per pair and the FFM's F vectors
per feature.  Entries of one field are sum-pooled; M[g][f] is M[f][g] transposed and M[f][f] is 0.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = FmFM(train, 16).learnWith(HipFmFM.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.m

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi, metrics


def identity_matrices(num_fields, num_factor):
    """M of a new model, (F, F, k, k): I for every pair f != g, 0 on the diagonal blocks."""
    m = np.zeros((num_fields, num_fields, num_factor, num_factor))
    m[:] = np.eye(num_factor)
    m[np.arange(num_fields), np.arange(num_fields)] = 0.0
    return m


class FmFMModel:
    """w0, w [n + 1], v [n + 1, k] and the field matrices m [F, F, k, k] on the device (fmhip_fmfm_model_t).  A new model has
    v = w = w0 = 0 and m[f][g] = I for f != g; FmFM.learnWith draws v."""

    def __init__(self, num_attribute, num_fields, num_factor, device=0, stream=None):
        self.num_attribute, self.num_fields, self.num_factor, self.device = int(num_attribute), int(num_fields), int(num_factor), int(device)
        h = C.c_void_p()
        _ffi.check(_ffi.load().fmhip_fmfm_model_create(self.device, self.num_attribute, self.num_fields, self.num_factor, stream, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    @property
    def padded_factors(self):
        kp = C.c_int32()
        _ffi.check(_ffi.load().fmhip_fmfm_model_info(self._h, None, None, None, C.byref(kp)))
        return kp.value

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

    def predict(self, dataset):
        """The margins yhat of the rows (fmhip_fmfm_predict), float64."""
        yh = np.zeros(dataset.size)
        _ffi.check(_ffi.load().fmhip_fmfm_predict(self._h, dataset.handle, _ffi.ptr(yh)))
        return yh

    def computeRMSE(self, dataset):
        return float(np.sqrt(np.mean((self.predict(dataset) - dataset.y) ** 2))) if dataset.size else 0.0

    def computeLogLoss(self, dataset):
        """Mean log-loss of sigmoid(predict) against t = [y > 0]: max(yhat, 0) - t yhat + log1p(exp(-|yhat|))."""
        if not dataset.size:
            return 0.0
        yh, t = self.predict(dataset), dataset.y > 0
        return float(np.mean(np.maximum(yh, 0.0) - t * yh + np.log1p(np.exp(-np.abs(yh)))))

    def computeAUC(self, dataset):
        """ROC AUC of the predictions against t = [y > 0], exact, ties one half (sparkfm_amd.metrics.auc)."""
        return metrics.auc(self.predict(dataset), dataset.y, device=self.device)["auc"]

    def computeAccuracy(self, dataset):
        if not dataset.size:
            return 0.0
        return float(((self.predict(dataset) >= 0) == (dataset.y > 0)).mean())

    def close(self):
        if self._h is not None:
            _ffi.load().fmhip_fmfm_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipFmFM:
    """The FmFM learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the field matrices and w0 every batch.
    field_matrices=False never steps m (with m = I: the plain FM on rows of one entry per field); linear=False never steps w0 and w."""

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regm=0.0, linear=True, field_matrices=True,
                 maxIteration=10, seed=0, adagrad_eps=1e-10, adagrad_init=1.0):
        self.loss_code, self.opt_code = _ffi.loss_code(loss), _ffi.optimizer_code(optimizer)
        self.adagrad_eps, self.adagrad_init = _ffi.adagrad_settings(adagrad_eps, adagrad_init)
        for name, x in (("eta", eta), ("reg0", reg0), ("regw", regw), ("regv", regv), ("regm", regm)):
            if not (np.isfinite(x) and x >= 0):
                raise ValueError("%s must be finite and >= 0, not %r" % (name, x))
        for name, x in (("linear", linear), ("field_matrices", field_matrices)):
            if not isinstance(x, bool):
                raise ValueError("%s must be True or False, not %r" % (name, x))
        self.loss, self.optimizer, self.linear, self.field_matrices = loss, optimizer, linear, field_matrices
        self.eta, self.rates = float(eta), (float(reg0), float(regw), float(regv), float(regm))
        self.maxIteration, self.seed = int(maxIteration), int(seed)
        self.last_stats = None

    @classmethod
    def run(cls, **kw):
        return cls(**kw)

    def _set_rule(self, model):
        L = _ffi.load()
        _ffi.check(L.fmhip_fmfm_model_set_rule(model.handle, self.loss_code, self.opt_code, self.adagrad_eps, self.adagrad_init))
        _ffi.check(L.fmhip_fmfm_model_set_linear(model.handle, int(self.linear)))
        _ffi.check(L.fmhip_fmfm_model_set_field_matrices(model.handle, int(self.field_matrices)))

    def step(self, model, dataset, batch, stats=True):
        """One mini-batch step (fmhip_fmfm_step) -> the batch's statistics (None with stats=False: no host synchronisation)."""
        self._set_rule(model)
        st = _ffi.Stats()
        _ffi.check(_ffi.load().fmhip_fmfm_step(model.handle, dataset.handle, int(batch), self.eta, *self.rates, C.byref(st) if stats else None))
        self.last_stats = st.as_dict() if stats else None
        return self.last_stats

    def learn(self, model, dataset, order=None):
        """One epoch (fmhip_fmfm_epoch) over the batches in `order` (None: ascending) -> model."""
        self._set_rule(model)
        st = _ffi.Stats()
        o = None if order is None else np.ascontiguousarray(order, np.int64)
        if o is not None and o.shape != (dataset.n_batches,):
            raise ValueError("order must hold one id per batch (%d)" % dataset.n_batches)
        _ffi.check(_ffi.load().fmhip_fmfm_epoch(model.handle, dataset.handle, self.eta, *self.rates, _ffi.ptr(o), C.byref(st)))
        self.last_stats = st.as_dict()
        return model

    def fit(self, model, dataset):
        """maxIteration epochs over the batches in ascending order."""
        for _ in range(self.maxIteration):
            self.learn(model, dataset)
        return model


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
