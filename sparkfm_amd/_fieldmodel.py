"""What the field models' wrappers share (ffm, fwfm, fmfm, deepfm, dcn, autoint): a model base over the handle — scoring, close — and
a learner base — the argument checks, the rule, step, learn, fit.  A subclass names its C functions (`_prefix`: fmhip_<model>) and, for
the five models with an array of their own, the switch that steps it (`_flag`) and its regulariser (`_reg`)."""
import ctypes as C

import numpy as np

from . import _ffi, metrics


class FieldModel:
    _prefix = None          # "fmhip_fwfm": the model's functions are <_prefix>_model_create, ..., <_prefix>_predict
    _info_tail = 0          # the outputs <_prefix>_model_info has behind padded_factors

    def _call(self, name, *args):
        _ffi.check(getattr(_ffi.load(), "%s_%s" % (self._prefix, name))(*args))

    def _create(self, num_attribute, num_fields, num_factor, device, stream, *own):
        """The handle: <_prefix>_model_create(device, n, F, k, *own, stream, &h)."""
        self.num_attribute, self.num_fields, self.num_factor, self.device = int(num_attribute), int(num_fields), int(num_factor), int(device)
        h = C.c_void_p()
        self._call("model_create", self.device, self.num_attribute, self.num_fields, self.num_factor, *own, stream, C.byref(h))
        self._h = h

    @property
    def handle(self):
        return self._h

    @property
    def padded_factors(self):
        kp = C.c_int32()
        self._call("model_info", self._h, None, None, None, C.byref(kp), *[None] * self._info_tail)
        return kp.value

    def predict(self, dataset):
        """The margins yhat of the rows (<_prefix>_predict), float64."""
        yh = np.zeros(dataset.size)
        self._call("predict", self._h, dataset.handle, _ffi.ptr(yh))
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
            getattr(_ffi.load(), self._prefix + "_model_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pointers(arrays):
    """A C array of the arrays' addresses (the per-layer arguments of the dense models)."""
    return (C.c_void_p * len(arrays))(*[_ffi.ptr(x) for x in arrays])


class FieldLearner:
    _prefix = None          # as FieldModel's
    _flag = None            # "field_weights": the argument and attribute that steps the model's own array, and <_prefix>_model_set_<_flag>
    _reg = None             # "regr": its regulariser, the last of self.rates

    def _setup(self, loss, optimizer, eta, reg0, regw, regv, regx, linear, flag, maxIteration, adagrad_eps, adagrad_init):
        self.loss_code, self.opt_code = _ffi.loss_code(loss), _ffi.optimizer_code(optimizer)
        self.adagrad_eps, self.adagrad_init = _ffi.adagrad_settings(adagrad_eps, adagrad_init)
        for name, x in (("eta", eta), ("reg0", reg0), ("regw", regw), ("regv", regv), (self._reg, regx)):
            if not (np.isfinite(x) and x >= 0):
                raise ValueError("%s must be finite and >= 0, not %r" % (name, x))
        for name, x in (("linear", linear), (self._flag, flag)):
            if not isinstance(x, bool):
                raise ValueError("%s must be True or False, not %r" % (name, x))
        self.loss, self.optimizer, self.linear = loss, optimizer, linear
        setattr(self, self._flag, flag)
        self.eta, self.rates = float(eta), (float(reg0), float(regw), float(regv), float(regx))
        self.maxIteration = int(maxIteration)
        self.last_stats = None

    @classmethod
    def run(cls, **kw):
        return cls(**kw)

    def _call(self, name, *args):
        _ffi.check(getattr(_ffi.load(), "%s_%s" % (self._prefix, name))(*args))

    def _set_rule(self, model):
        self._call("model_set_rule", model.handle, self.loss_code, self.opt_code, self.adagrad_eps, self.adagrad_init)
        self._call("model_set_linear", model.handle, int(self.linear))
        if self._flag:
            self._call("model_set_" + self._flag, model.handle, int(getattr(self, self._flag)))

    def step(self, model, dataset, batch, stats=True):
        """One mini-batch step (<_prefix>_step) -> the batch's statistics (None with stats=False: no host synchronisation)."""
        self._set_rule(model)
        st = _ffi.Stats()
        self._call("step", model.handle, dataset.handle, int(batch), self.eta, *self.rates, C.byref(st) if stats else None)
        self.last_stats = st.as_dict() if stats else None
        return self.last_stats

    def learn(self, model, dataset, order=None):
        """One epoch (<_prefix>_epoch) over the batches in `order` (None: ascending) -> model."""
        self._set_rule(model)
        st = _ffi.Stats()
        o = None if order is None else np.ascontiguousarray(order, np.int64)
        if o is not None and o.shape != (dataset.n_batches,):
            raise ValueError("order must hold one id per batch (%d)" % dataset.n_batches)
        self._call("epoch", model.handle, dataset.handle, self.eta, *self.rates, _ffi.ptr(o), C.byref(st))
        self.last_stats = st.as_dict()
        return model

    def fit(self, model, dataset):
        """maxIteration epochs over the batches in ascending order."""
        for _ in range(self.maxIteration):
            self.learn(model, dataset)
        return model
