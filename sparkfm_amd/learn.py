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


class HipFTRL(HipSGD):
    """``HipSGD`` under FTRL-Proximal with L1 (include/fmhip_ftrl.h; McMahan et al., the `ftrl` optimizer of xLearn and alphaFM):
    per-coordinate rates like AdaGrad's plus an L1 term that leaves most of a wide model EXACTLY zero (``FMModel.nonzeros()``).

        fm = FM(train, 4, maxIteration=20).learnWith(HipFTRL.run(loss="logistic", alpha=0.1, beta=0.05, l1w=1.0, l2w=1e-4, l2v=1e-4))

    `alpha`: the step size (the training calls' eta).  `beta`: added to sqrt(n) in every rate.  `l1w`, `l1v`: the L1 of the linear
    weights and of the factors (w0 has none).  `l2_0`, `l2w`, `l2v`: the L2 of the rule's closed form (the calls' reg0 / regw /
    regv — not a decay: a parameter whose gradient is zero keeps every bit, so a batch that touches few rows of a wide model
    updates those rows only, whatever the regularisation).  `ftrl_init`: what the accumulators n start at.  Per parameter, with g
    the batch's mean gradient:  n' = n + g^2;  zeta' = zeta + alpha g - (sqrt(n') - sqrt(n)) theta;
    theta' = 0 if |zeta'| <= alpha l1 else -(zeta' - sign(zeta') alpha l1) / (beta + sqrt(n') + alpha l2).
    With l1 = l2 = 0 that is AdaGrad with eps = beta.  Note that an L1 on V beyond its initial scale zeroes EVERY factor row — the
    gradient of v_i vanishes where all of V is zero — so l1v is for models whose factors have grown; l1w is the usual knob.
    `loss`, `pairs`, `shuffle_seed`: as ``HipSGD``.  ``learn`` / ``step`` are inherited and take a ``DataSet`` (weighted too) or a
    ``RelationalData``; both put the rule on the model first (the same settings again keep its state; changed ones restart it)."""

    def __init__(self, alpha=0.1, beta=1.0, l1w=0.0, l1v=0.0, l2_0=0.0, l2w=0.0, l2v=0.0, ftrl_init=0.0, loss="squared", pairs=False,
                 shuffle_seed=None):
        import math
        for name, x in (("alpha", alpha), ("l2_0", l2_0), ("l2w", l2w), ("l2v", l2v)):
            if not (math.isfinite(float(x)) and float(x) >= 0.0):
                raise ValueError("%s must be finite and >= 0, not %r" % (name, x))
        self.alpha = self.eta = float(alpha)
        self.l2_0, self.l2w, self.l2v = float(l2_0), float(l2w), float(l2v)
        self.reg0, self.regw, self.regv = self.l2_0, self.l2w, self.l2v
        self.rule = _ffi.FtrlRule(loss, pairs, beta, ftrl_init, l1w, l1v).publish(self)
        self.optimizer = "ftrl"
        self.shuffle_seed = shuffle_seed
        self._epoch = 0
        self.last_stats = None


class HipSGDA(HipSGD):
    """``HipSGD`` whose regularisers are learned while it trains (include/fmhip_sgda.h; libFM's ``-method sgda -validation``; Rendle,
    "Learning recommender systems with adaptive regularization"): a lambda_w per feature group and a lambda_v per (factor, feature
    group), each stepped after every train batch along the gradient of a held-out batch's loss.  Nothing to grid-search.

        sgda = HipSGDA.run(validation=val, groups=Metadata.fromFields((n_users, n_items)), eta=0.05)
        fm = FM(train, k, maxIteration=E).learnWith(sgda)
        sgda.state["lambda_w"], sgda.last_validation_stats

    `validation`: a DataSet made like the train set (it needs its transposes: not ``scoring=True``); step t of the run takes its batch
    t mod n_batches.  `groups`: None (one group), a ``Metadata`` or an int array with one group id per feature ROW — the model has
    num_attribute + 1 rows (quirk Q1's spare slot); an array or Metadata exactly one entry short is padded with its last id.
    `eta_lambda`: the regularisers' step size relative to eta (None: eta, libFM's choice); lambda <- max(0, lambda + eta_lambda eta S).
    `init_lambda`: where every lambda starts.  ``validation=None`` with ``eta_lambda=0`` is SGD with a FIXED regulariser per group, and
    `init_lambda` may then also be a pair ``(lambda_w[G], lambda_v[k][G])``.  `reg0` regularises w0 as in ``HipSGD``.
    `loss`, `shuffle_seed`: as ``HipSGD``.  Plain SGD on single, unweighted rows of a ``DataSet`` only: no AdaGrad / FTRL, no pairs,
    no ``RelationalData`` (FmhipError, FMHIP_ERR_UNSUPPORTED).  The handle is made by the first ``learn`` / ``step`` for a model and
    remade when the model changes; ``close()`` frees it."""

    def __init__(self, validation=None, groups=None, eta=0.05, eta_lambda=None, init_lambda=0.0, reg0=0.0, loss="squared", shuffle_seed=None):
        import math
        super().__init__(eta=eta, reg0=reg0, shuffle_seed=shuffle_seed, loss=loss)
        self.eta_lambda = self.eta if eta_lambda is None else float(eta_lambda)
        if not (math.isfinite(self.eta_lambda) and self.eta_lambda >= 0.0):
            raise ValueError("eta_lambda must be finite and >= 0, not %r" % (eta_lambda,))
        if validation is None and self.eta_lambda != 0.0:
            raise ValueError("eta_lambda = %r needs a validation set: pass validation=, or eta_lambda=0 for fixed per-group regularisation" % self.eta_lambda)
        if validation is not None and getattr(validation, "scoring", False):
            raise ValueError("the validation set must keep its transposes: make it without scoring=True")
        self.validation = validation
        self.groups, self.n_groups = None, 1
        if groups is not None:
            from .metadata import Metadata
            if isinstance(groups, Metadata):
                table, n_groups = groups.attrGroup, groups.numAttrGroups
            else:
                table = np.asarray(groups)
                if table.ndim != 1 or (len(table) and not np.issubdtype(table.dtype, np.integer)):
                    raise TypeError("groups must be a Metadata or a 1-d integer array (one group id per feature row)")
                if len(table) and table.min() < 0:
                    raise ValueError("feature %d has group id %d: ids are >= 0" % (int(np.argmin(table)), int(table.min())))
                n_groups = int(table.max()) + 1 if len(table) else 1
            if n_groups > _ffi.SGDA_MAX_GROUPS:
                raise ValueError("%d feature groups: at most %d (FMHIP_SGDA_MAX_GROUPS)" % (n_groups, _ffi.SGDA_MAX_GROUPS))
            self.groups, self.n_groups = np.ascontiguousarray(table, np.int32), int(n_groups)
        self._init_pair = None
        if isinstance(init_lambda, (tuple, list)):
            if validation is not None or self.eta_lambda != 0.0:
                raise ValueError("a (lambda_w, lambda_v) pair as init_lambda goes with validation=None and eta_lambda=0 (fixed regularisation)")
            lw, lv = init_lambda
            self._init_pair = (np.array(lw, np.float64), np.array(lv, np.float64))
            self.init_lambda = 0.0
        else:
            self.init_lambda = float(init_lambda)
            if not (math.isfinite(self.init_lambda) and self.init_lambda >= 0.0):
                raise ValueError("init_lambda must be finite and >= 0, not %r" % (init_lambda,))
        self._h = None
        self._for = None            # the model handle's value the SGDA handle was made for
        self._keep = None
        self.last_validation_stats = None

    def _handle(self, fm):
        L = _ffi.load()
        if self._h is not None and self._for != fm.handle.value:
            self.close()
        if self._h is None:
            n1 = fm.num_attribute + 1
            if self.groups is None:
                table = np.zeros(n1, np.int32)
            elif len(self.groups) == n1 - 1:
                table = np.ascontiguousarray(np.append(self.groups, self.groups[-1] if n1 > 1 else 0), np.int32)
            elif len(self.groups) == n1:
                table = self.groups
            else:
                raise ValueError("groups holds %d ids but the model has num_attribute + 1 = %d feature rows" % (len(self.groups), n1))
            self.rule.set_on(fm.handle)
            h = C.c_void_p()
            _ffi.check(L.fmhip_sgda_create(fm.handle, _ffi.ptr(table), n1, self.n_groups, self.init_lambda, self.init_lambda, C.byref(h)))
            self._h, self._for, self._k, self._keep = h, fm.handle.value, fm.num_factor, fm
            if self._init_pair is not None:
                try:
                    self.set_state(*self._init_pair)
                except Exception:
                    self.close()
                    raise
        return self._h

    def _data(self, dataset):
        if isinstance(dataset, RelationalData):
            raise _ffi.FmhipError(-5, "SGDA does not take relational data yet: expand() it and train on the flat rows, or use HipSGD")
        return dataset.handle

    def _metric(self, st, fm=None):
        """A validation stats block -> its dict plus `rmse` over its rows (squared loss: the validation loss, for free) and, for an
        epoch under the logistic loss, `logloss`: one scoring pass over the validation set after the epoch (the training forward
        sums residuals, not log-likelihoods)."""
        d = st.as_dict()
        d["rmse"] = float(np.sqrt(d["sse"] / d["rows"])) if d["rows"] > 0 else float("nan")
        if fm is not None and self.loss == "logistic":
            d["logloss"] = fm.computeLogLoss(self.validation)
        return d

    def learn(self, fm, dataset):
        L = _ffi.load()
        dh = self._data(dataset)
        self.rule.set_on(fm.handle)
        h = self._handle(fm)
        order = self.batch_order(dataset.n_batches)
        st, sv = _ffi.Stats(), _ffi.Stats()
        val = self.validation
        _ffi.check(L.fmhip_sgda_epoch(h, dh, None if val is None else val.handle, self.eta, self.eta_lambda, self.reg0, _ffi.ptr(order),
                                      C.byref(st), C.byref(sv)))
        fm._device_updated()
        self._epoch += 1
        self.last_stats = st.as_dict()
        self.last_validation_stats = None if val is None else self._metric(sv, fm)
        return fm

    def step(self, fm, dataset, batch, val_batch=None, want_stats=True):
        """A single step (fmhip_sgda_step): train batch `batch`, validation batch `val_batch` (None: the handle's step counter mod the
        validation set's batches).  -> (train stats, validation stats) dicts, or None."""
        L = _ffi.load()
        dh = self._data(dataset)
        self.rule.set_on(fm.handle)
        h = self._handle(fm)
        val = self.validation
        if val is not None and val_batch is None:
            val_batch = self.state["steps"] % max(val.n_batches, 1)
        st, sv = _ffi.Stats(), _ffi.Stats()
        _ffi.check(L.fmhip_sgda_step(h, dh, batch, None if val is None else val.handle, 0 if val_batch is None else int(val_batch), self.eta,
                                     self.eta_lambda, self.reg0, C.byref(st) if want_stats else None,
                                     C.byref(sv) if want_stats and val is not None else None))
        fm._device_updated()
        if not want_stats:
            return None
        return st.as_dict(), (None if val is None else self._metric(sv))

    def _need(self):
        if self._h is None:
            raise RuntimeError("HipSGDA has no handle yet: it is made by the first learn(fm, dataset) or step")
        return self._h

    @property
    def state(self):
        """dict of lambda_w (G,), lambda_v (k, G) and steps (the steps taken: the validation batches' counter)."""
        h = self._need()
        lw, lv, steps = np.empty(self.n_groups), np.empty((self._k, self.n_groups)), C.c_int64()
        _ffi.check(_ffi.load().fmhip_sgda_get_lambda(h, _ffi.ptr(lw), _ffi.ptr(lv)))
        _ffi.check(_ffi.load().fmhip_sgda_info(h, None, None, C.byref(steps)))
        return dict(lambda_w=lw, lambda_v=lv, steps=int(steps.value))

    def set_state(self, lambda_w, lambda_v):
        """lambda_w (G,) and lambda_v (k, G), finite and >= 0 (the library refuses anything else and keeps what it had)."""
        lw, lv = np.ascontiguousarray(lambda_w, np.float64), np.ascontiguousarray(lambda_v, np.float64)
        self._need()
        if lw.shape != (self.n_groups,) or lv.shape != (self._k, self.n_groups):
            raise ValueError("lambda_w must have shape (%d,) and lambda_v (%d, %d)" % (self.n_groups, self._k, self.n_groups))
        _ffi.check(_ffi.load().fmhip_sgda_set_lambda(self._h, _ffi.ptr(lw), _ffi.ptr(lv)))

    def last_sums(self):
        """(S_w (G,), S_v (k, G)) of the last step that had a validation batch, fp64: d(validation loss)/d lambda = -eta S."""
        h = self._need()
        sw, sv = np.empty(self.n_groups), np.empty((self._k, self.n_groups))
        _ffi.check(_ffi.load().fmhip_sgda_last_sums(h, _ffi.ptr(sw), _ffi.ptr(sv)))
        return sw, sv

    @property
    def group_counts(self):
        """int64 [G]: the feature rows of every group."""
        counts = np.empty(self.n_groups, np.int64)
        _ffi.check(_ffi.load().fmhip_sgda_info(self._need(), None, _ffi.ptr(counts), None))
        return counts

    def close(self):
        if self._h is not None:
            _ffi.load().fmhip_sgda_destroy(self._h)
        self._h, self._for, self._keep = None, None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


class HipMCMC(FMLearn):
    """Bayesian FM by Gibbs sampling on the ALS column walk (include/fmhip_mcmc.h; libFM's MCMC learner, of which the reference's
    ``ALS.scala`` is the cut-down copy): one ``learn`` = one Gibbs sweep in fp64.  No learning rate and no regularisers to tune:
    the noise precision alpha and, per parameter group, the regulariser lambda and the prior mean mu are sampled; the prediction is
    the average over the draws.

        mcmc = HipMCMC.run(test=test, burn_in=15)
        fm = FM(train, k, maxIteration=40).learnWith(mcmc)       # fm holds the LAST draw
        mcmc.predictions(); mcmc.computeRMSE()                   # the averaged prediction of the 25 kept draws on `test`

    `seed`: the key of the counter-based generator (the same seed gives the same bits, whatever walk the sweep takes).  `test`: a
    DataSet (single batch, not scoring-only) whose predictions are averaged, or None.  `burn_in`: the running average is reset
    once, after that many epochs.  `sample=False`: no draws at all — the conditional means under the state as set (with alpha = 1,
    mu = 0, lambda = (regw, regv ...) that is ``HipALS``, bit for bit).  Priors (libFM's defaults): reg0 = 0, init_lambda = 1,
    alpha_0 = beta_0 = alpha_lambda = beta_lambda = gamma_0 = 1, mu_0 = 0.  The handle is made on the first ``learn`` for a
    (model, dataset) pair and remade when either changes; ``close()`` frees it.  Needs a single-batch DataSet like ``HipALS``.

    This class takes flat rows; a ``RelationalData`` is swept by blocks, never expanded, by its subclass ``HipBlockMCMC``.

    `task` (include/fmhip_mcmc_task.h): "regression", or "classification" — binary labels [y > 0] by the probit link: every epoch
    trains on latent targets drawn from truncated normals (``latent_targets()``), alpha stays 1, and ``predictions()`` /
    ``last_predictions()`` are PROBABILITIES Phi(yhat), scored by ``computeLogLoss()``, ``computeAccuracy()`` and ``computeAUC()``
    (``computeRMSE()`` raises).  Afterwards `fm` is the last draw and ``fm.predict`` its probit score: the probability is Phi(yhat),
    not the logistic sigmoid, so ``FMModel.computeAUC`` and ``computeAccuracy`` apply to it and ``FMModel.computeLogLoss`` does not.
    `clip` (regression only): None, (lo, hi), or "labels" — the train labels' min and max, taken when the handle is made: every
    draw's test prediction is clamped to that range before it is averaged (libFM's way; off unless asked for).

    `groups` (include/fmhip_mcmc_groups.h): None, a ``Metadata`` or an int array with one attribute-group id per feature (at least
    the model's num_attribute entries; what lies behind is not read).  lambda and mu are then sampled per (parameter group, attribute
    group) — users, items and context fields each get their own scale, as in libFM — ``state`` holds ``lambda`` and ``mu`` of
    shape (k + 1, G), and ``group_counts`` the trained features of every group."""

    PRIORS = ("reg0", "init_lambda", "alpha_0", "beta_0", "alpha_lambda", "beta_lambda", "gamma_0", "mu_0")

    TASKS = {"regression": _ffi.MCMC_REGRESSION, "classification": _ffi.MCMC_CLASSIFICATION}
    RELATIONAL = False          # HipBlockMCMC: the train set is a RelationalData, `test` may be one, groups may be "parts"

    def __init__(self, seed=0, test=None, burn_in=0, sample=True, task="regression", clip=None, groups=None, **priors):
        import math
        import operator
        self.groups, self.n_groups = None, 1
        if self.RELATIONAL and isinstance(groups, str) and groups == "parts":
            self.groups = "parts"       # (n_groups: the train set's parts, known when the handle is made)
        elif groups is not None:
            from .metadata import Metadata
            if isinstance(groups, Metadata):
                table, n_groups = groups.attrGroup, groups.numAttrGroups
            else:
                table = np.asarray(groups)
                if table.ndim != 1 or (len(table) and not np.issubdtype(table.dtype, np.integer)):
                    raise TypeError("groups must be a Metadata, a 1-d integer array (one group id per feature) or, with HipBlockMCMC, 'parts'")
                if len(table) and table.min() < 0:
                    raise ValueError("feature %d has group id %d: ids are >= 0" % (int(np.argmin(table)), int(table.min())))
                n_groups = int(table.max()) + 1 if len(table) else 1
            if n_groups > _ffi.MCMC_MAX_GROUPS:
                raise ValueError("%d attribute groups: at most %d (FMHIP_MCMC_MAX_GROUPS)" % (n_groups, _ffi.MCMC_MAX_GROUPS))
            self.groups, self.n_groups = np.ascontiguousarray(table, np.int32), int(n_groups)
        if not isinstance(task, str) or task not in self.TASKS:
            raise ValueError("task must be 'regression' or 'classification', not %r" % (task,))
        self.task = task
        if clip is not None and task == "classification":
            raise ValueError("clip goes with task='regression': a classification run's predictions are probabilities")
        if clip is not None and not (isinstance(clip, str) and clip == "labels"):
            try:
                if isinstance(clip, str):
                    raise TypeError
                lo, hi = clip
                clip = (float(lo), float(hi))
            except (TypeError, ValueError):
                raise ValueError("clip must be None, (lo, hi) or 'labels', not %r" % (clip,)) from None
            if not (math.isfinite(clip[0]) and math.isfinite(clip[1]) and clip[0] < clip[1]):
                raise ValueError("the clip range must be finite with lo < hi, not %r" % (clip,))
        self.clip = clip
        self.seed = operator.index(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64), not %r" % (seed,))
        self.burn_in = operator.index(burn_in)
        if self.burn_in < 0:
            raise ValueError("burn_in must be >= 0, not %d" % self.burn_in)
        if not isinstance(sample, bool):
            raise ValueError("sample must be True or False, not %r" % (sample,))
        self.sample = sample
        if isinstance(test, RelationalData) and not self.RELATIONAL:
            test.handle             # raises: this call takes flat rows
        if test is not None and getattr(test, "scoring", False):
            raise ValueError("the test set must keep its fp64 rows: make it without scoring=True")
        self.test = test
        unknown = sorted(set(priors) - set(self.PRIORS))
        if unknown:
            raise TypeError("unknown prior %r (known: %s)" % (unknown[0], ", ".join(self.PRIORS)))
        self.priors = dict(reg0=0.0, init_lambda=1.0, alpha_0=1.0, beta_0=1.0, alpha_lambda=1.0, beta_lambda=1.0, gamma_0=1.0, mu_0=0.0)
        for name, value in priors.items():
            value = float(value)
            ok = math.isfinite(value) and (True if name == "mu_0" else value >= 0.0 if name == "reg0" else value > 0.0)
            if not ok:
                raise ValueError("%s must be finite and > 0 (mu_0: finite; reg0: finite and >= 0), not %r" % (name, value))
            self.priors[name] = value
        self._h = None
        self._for = None            # the (model handle, dataset handle) values the MCMC handle was made for
        self._pending_state = None
        self.last_stats = None

    @classmethod
    def run(cls, seed=0, test=None, burn_in=0, sample=True, task="regression", clip=None, groups=None, **priors):
        return cls(seed=seed, test=test, burn_in=burn_in, sample=sample, task=task, clip=clip, groups=groups, **priors)

    def _handle(self, fm, dataset):
        L = _ffi.load()
        relational = self.RELATIONAL
        if relational and self.groups is not None and not isinstance(self.groups, str):
            raise ValueError("a RelationalData train set takes no group table: groups='parts' makes every part (relation 0, 1, ..., the plain part) "
                             "an attribute group — what relational.meta() names over expand()")
        mh, dh = fm.handle, dataset.rel_handle if relational else dataset.handle
        if self._h is not None and self._for != (mh.value, dh.value):
            self.close()
        if self._h is None:
            n = fm.num_attribute
            if relational:
                self.n_groups = len(dataset._parts()) if self.groups is not None else 1
            elif self.groups is not None and len(self.groups) < n:
                raise ValueError("groups holds %d ids but the model has num_attribute = %d" % (len(self.groups), n))
            opts = _ffi.McmcOpts(self.seed, 1 if self.sample else 0, *[self.priors[n] for n in self.PRIORS])
            h = C.c_void_p()
            clip = self.clip
            if clip == "labels":
                y = np.asarray(dataset.y, np.float64)
                if not len(y):
                    raise ValueError("clip='labels' needs a train set with rows")
                clip = (float(y.min()), float(y.max()))
            task = _ffi.McmcTaskOpts(self.TASKS[self.task], 0 if clip is None else 1, *(clip or (0.0, 0.0)))
            if relational:
                rel_test = isinstance(self.test, RelationalData)
                _ffi.check(L.fmhip_mcmc_create_relational(mh, dh, self.test.rel_handle if rel_test else None,
                                                          None if self.test is None or rel_test else self.test.handle, C.byref(opts), C.byref(task),
                                                          0 if self.groups is None else 1, C.byref(h)))
            else:
                _ffi.check(L.fmhip_mcmc_create_task(mh, dh, None if self.test is None else self.test.handle, C.byref(opts), C.byref(task), C.byref(h)))
            self._h, self._for, self._k, self._n_train = h, (mh.value, dh.value), fm.num_factor, dataset.size
            self._keep = (fm, dataset)      # the handle borrows both
            if self.groups is not None and not relational:
                table = np.ascontiguousarray(self.groups[:n])
                rc = L.fmhip_mcmc_set_groups(h, _ffi.ptr(table), n, self.n_groups)
                if rc != 0:
                    self.close()
                    _ffi.check(rc)
            if self._pending_state is not None:
                self.state = self._pending_state
                self._pending_state = None
        return self._h

    def learn(self, fm, dataset):
        if isinstance(dataset, RelationalData) != self.RELATIONAL:
            if self.RELATIONAL:
                raise TypeError("HipBlockMCMC sweeps the blocks of a RelationalData, not flat rows: HipMCMC takes a %s" % type(dataset).__name__)
            dataset.handle          # raises: this call takes flat rows
        L = _ffi.load()
        h = self._handle(fm, dataset)
        st = _ffi.McmcStats()
        _ffi.check(L.fmhip_mcmc_epoch(h, C.byref(st)))
        fm._device_updated()
        self.last_stats = st.as_dict()
        if self.burn_in > 0 and st.iterations == self.burn_in:
            _ffi.check(L.fmhip_mcmc_reset_average(h))
        return fm

    def _need(self):
        if self._h is None:
            raise RuntimeError("HipMCMC has no handle yet: it is made by the first learn(fm, dataset)")
        return self._h

    @property
    def state(self):
        """dict of alpha, lambda (k + 1: group 0 = w, 1 + f = factor f), mu (k + 1), iterations; with `groups` lambda and mu are
        (k + 1, G): a row per parameter group, a column per attribute group."""
        h = self._need()
        alpha, it = C.c_double(), C.c_int64()
        lam, mu = np.empty(self._state_shape()), np.empty(self._state_shape())
        get = _ffi.load().fmhip_mcmc_get_state if self.groups is None else _ffi.load().fmhip_mcmc_get_group_state
        _ffi.check(get(h, C.byref(alpha), _ffi.ptr(lam), _ffi.ptr(mu), C.byref(it)))
        return dict(alpha=alpha.value, **{"lambda": lam, "mu": mu, "iterations": int(it.value)})

    @state.setter
    def state(self, value):
        """(alpha, lambda, mu) or a dict with those keys; before the first learn it is kept and set when the handle is made."""
        if isinstance(value, dict):
            value = (value["alpha"], value["lambda"], value["mu"])
        alpha, lam, mu = value
        if self._h is None:
            self._pending_state = (float(alpha), np.array(lam, np.float64), np.array(mu, np.float64))
            return
        lam, mu = np.ascontiguousarray(lam, np.float64), np.ascontiguousarray(mu, np.float64)
        if lam.shape != self._state_shape() or mu.shape != self._state_shape():
            raise ValueError("lambda and mu must have shape %r (k + 1%s)" % (self._state_shape(), "" if self.groups is None else ", G"))
        put = _ffi.load().fmhip_mcmc_set_state if self.groups is None else _ffi.load().fmhip_mcmc_set_group_state
        _ffi.check(put(self._h, float(alpha), _ffi.ptr(lam), _ffi.ptr(mu)))

    def _state_shape(self):
        return (self._k + 1,) if self.groups is None else (self._k + 1, self.n_groups)

    @property
    def group_counts(self):
        """int64 [G]: m_a, the trained features of attribute group a (quirk Q1's last slot never counts); [m] without groups."""
        g = C.c_int32()
        _ffi.check(_ffi.load().fmhip_mcmc_group_info(self._need(), C.byref(g), None))
        counts = np.empty(g.value, np.int64)
        _ffi.check(_ffi.load().fmhip_mcmc_group_info(self._h, None, _ffi.ptr(counts)))
        return counts

    def reset_average(self):
        _ffi.check(_ffi.load().fmhip_mcmc_reset_average(self._need()))

    def _predictions(self):
        if self.test is None:
            raise RuntimeError("HipMCMC was made without a test set")
        mean, last, draws = np.empty(self.test.size), np.empty(self.test.size), C.c_int64()
        _ffi.check(_ffi.load().fmhip_mcmc_predictions(self._need(), _ffi.ptr(mean), _ffi.ptr(last), C.byref(draws)))
        return mean, last, int(draws.value)

    def predictions(self):
        """The test rows' predictions averaged over the draws since the burn-in ended (or the last reset_average)."""
        return self._predictions()[0]

    def last_predictions(self):
        """The test rows' predictions under the last draw (what ``fm.predict(test)`` gives in fp64)."""
        return self._predictions()[1]

    @property
    def draws(self):
        return self._predictions()[2]

    def latent_targets(self):
        """The targets the last epoch trained on, one per train row: a classification run's y* (the label's sign times a truncated
        normal around the row's score; +-1 in the first epoch); the labels on a regression run and before the first epoch."""
        out = np.empty(self._n_train if self._h is not None else 0)
        _ffi.check(_ffi.load().fmhip_mcmc_latent_targets(self._need(), _ffi.ptr(out)))
        return out

    def _classes(self, what):
        if self.task != "classification":
            raise ValueError("%s scores a classification run's probabilities: this run's task is %r (see computeRMSE)" % (what, self.task))
        return self.predictions(), np.asarray(self.test.y) > 0

    def computeLogLoss(self):
        """Mean log-loss of the averaged probabilities against the test classes [y > 0] (probabilities kept 1e-15 away from 0 and 1)."""
        p, t = self._classes("computeLogLoss")
        p = np.clip(p, 1e-15, 1.0 - 1e-15)
        return float(-np.mean(np.where(t, np.log(p), np.log1p(-p)))) if len(p) else 0.0

    def computeAccuracy(self):
        """Share of the test rows whose averaged probability is on the label's side of 1/2."""
        p, t = self._classes("computeAccuracy")
        return float(np.mean((p > 0.5) == t)) if len(p) else 0.0

    def computeAUC(self):
        """ROC AUC of the averaged probabilities against the test classes (``sparkfm_amd.metrics.auc``)."""
        from . import metrics
        p, t = self._classes("computeAUC")
        return metrics.auc(p, t.astype(np.float32), device=self.test.device)["auc"]

    def computeRMSE(self):
        """RMSE of the averaged prediction against the test labels (regression)."""
        if self.task == "classification":
            raise ValueError("a classification run's predictions are probabilities: score them with computeLogLoss, computeAccuracy or computeAUC")
        mean = self.predictions()
        return float(np.sqrt(np.mean((mean - self.test.y.astype(np.float64)) ** 2))) if len(mean) else 0.0

    def close(self):
        if self._h is not None:
            _ffi.load().fmhip_mcmc_destroy(self._h)
            self._h, self._for, self._keep = None, None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipBlockMCMC(HipMCMC):
    """``HipMCMC`` over a ``RelationalData`` (single batch), swept BY BLOCKS (include/fmhip_mcmc_relational.h; Rendle, "Scaling
    Factorization Machines to Relational Data") — ``expand()`` is never built: a block column costs one entry per block row instead of
    one per data row that references it, its sums taken from per-block-row caches.  Same seed, same random numbers as ``HipMCMC`` on
    ``expand()``; the two differ by rounding.

        mcmc = HipBlockMCMC.run(test=held_out, burn_in=15, groups="parts")
        fm = FM(ratings, k, maxIteration=40).withRelation([users, items]).learnWith(mcmc)

    Everything is ``HipMCMC``'s — tasks, clip, priors, state, predictions, scores — except: `test` is a ``RelationalData`` (normally the
    train set's blocks under ``Relation.remap``) or a flat DataSet; `groups` is None or "parts" — every part (relation 0, 1, ..., the plain
    part) is an attribute group, as ``relational.meta()`` names them over ``expand()``, and ``state`` is (k + 1, parts); a table is not
    taken.  The parts' feature-id ranges must not interleave (the block sweep walks part after part, the flat one ascending ids)."""

    RELATIONAL = True
