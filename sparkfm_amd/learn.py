"""FMLearn plug-in point and the HIP mini-batch SGD learner.

``FMLearn.learn(fm, dataset): FMModel`` is the reference's abstract learner
(S/fm/FMLearn.scala:10-12), invoked once per iteration by the fit loop
(S/fm/impl/FactorizationMachines.scala:45).  ``HipSGD`` is the MI355X learner behind it;
``HipSGD.run(...)`` mirrors ``ALS.run()`` (S/fm/lib/ALS.scala:202-208).
"""
import ctypes as C

import numpy as np

from . import _ffi
from .relational import RelationalData


class FMLearn:
    def learn(self, fm, dataset):
        raise NotImplementedError


class HipSGD(FMLearn):
    """One ``learn`` call = one epoch of mini-batch SGD on the GPU (all batches of `dataset`).

    SparkFM has no SGD learner (its only learner is ALS); the update rule is this build's:
        theta <- theta - eta * (sum_{r in batch} e_r h_r(theta) / |batch| + reg * theta)
    with e, h from S/fm/lib/ALS.scala:142-144 and :56-58/:40/:21.  The regularisers are the
    learner's own (the model's regv = 10 default is an ALS ridge term — quirk Q5).
    `loss`: "squared" (e = yhat - y, regression) or "logistic" (e = sigmoid(yhat) - [y > 0]: a binary
    classifier of labels {0,1} or {-1,+1}, the gradient of the mean log-loss; fmhip_model_set_loss).
    `optimizer`: "sgd" (the rule above) or "adagrad" (torch.optim.Adagrad with lr = eta, weight_decay = reg: every
    parameter keeps an accumulator n, started at `adagrad_init`; g_hat = g/|batch| + reg*theta, n += g_hat^2,
    theta -= eta*g_hat / (sqrt(n) + adagrad_eps); fmhip_model_set_optimizer).
    `pairs`: True trains on PAIRS of rows (pairwise ranking; fmhip_model_set_pairing): rows 2j and 2j+1 of a batch are one
    example and the loss is applied to their difference — with loss="logistic" and the preferred row first (label 1 / 0,
    ``DataSet.from_pairs``) this is BPR, -log sigmoid(yhat_preferred - yhat_other).  The dataset needs an even number of rows
    and an even batch_rows.
    `learn` and `step` set all three on the model before they train (the same AdaGrad settings again keep its accumulators).
    Both also take a ``RelationalData`` (fmhip_relational_sgd_epoch / _step: every block walked once per step; not with pairs).
    """

    def __init__(self, eta=0.05, reg0=0.0, regw=0.0, regv=0.0, shuffle_seed=None, loss="squared", optimizer="sgd",
                 adagrad_eps=1e-10, adagrad_init=0.1, pairs=False):
        self.eta, self.reg0, self.regw, self.regv = float(eta), float(reg0), float(regw), float(regv)
        self.rule = _ffi.TrainRule(loss, optimizer, adagrad_eps, adagrad_init, pairs).publish(self)
        self.shuffle_seed = shuffle_seed
        self._epoch = 0
        self.last_stats = None

    @classmethod
    def run(cls, **kw):
        return cls(**kw)

    def batch_order(self, n_batches):
        """Visiting order of the (fixed, contiguous) mini-batches for the next epoch."""
        if self.shuffle_seed is None:
            return None
        rng = np.random.Generator(np.random.PCG64([self.shuffle_seed, self._epoch]))
        return rng.permutation(n_batches).astype(np.int64)

    def learn(self, fm, dataset):
        L = _ffi.load()
        order = self.batch_order(dataset.n_batches)
        st = _ffi.Stats()
        self.rule.set_on(fm.handle)
        if isinstance(dataset, RelationalData):
            _ffi.check(L.fmhip_relational_sgd_epoch(fm.handle, dataset.rel_handle, self.eta, self.reg0, self.regw, self.regv,
                                                    _ffi.ptr(order), C.byref(st)))
        else:
            _ffi.check(L.fmhip_sgd_epoch(fm.handle, dataset.handle, self.eta, self.reg0, self.regw, self.regv,
                                         _ffi.ptr(order), C.byref(st)))
        fm._device_updated()
        self._epoch += 1
        self.last_stats = st.as_dict()
        return fm

    def step(self, fm, dataset, batch, want_stats=True):
        """A single mini-batch step (fmhip_sgd_step)."""
        st = _ffi.Stats()
        self.rule.set_on(fm.handle)
        relational = isinstance(dataset, RelationalData)
        fn = _ffi.load().fmhip_relational_sgd_step if relational else _ffi.load().fmhip_sgd_step
        _ffi.check(fn(fm.handle, dataset.rel_handle if relational else dataset.handle, batch, self.eta, self.reg0, self.regw,
                      self.regv, C.byref(st) if want_stats else None))
        fm._device_updated()
        return st.as_dict() if want_stats else None


class HipALS(FMLearn):
    """The reference's own learner on the GPU: one ``learn`` = one ``ALS.learn`` pass
    (S/fm/lib/ALS.scala:15-75) in fp64, using the MODEL's regularisers ``fm.reg0/regw/regv`` as the
    reference does (:21,:40,:56; defaults 0, 0, 10).  ``HipALS.run()`` mirrors ``ALS.run()`` (:202-208).
    Needs a single-batch DataSet (``batch_rows=0``)."""

    @classmethod
    def run(cls):
        return cls()

    def learn(self, fm, dataset):
        _ffi.check(_ffi.load().fmhip_als_epoch(fm.handle, dataset.handle, fm.reg0, fm.regw, fm.regv))
        fm._device_updated()
        return fm
