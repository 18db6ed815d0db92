"""Model / FMModel — host mirror of S/Model.scala and S/fm/FMModel.scala.

``FMModel`` keeps the reference's public, mutable fields (w0, w, v, reg0, regw, regv) as
fp64 numpy arrays in the reference's layout — ``v`` is ``(num_factor, num_attribute+1)``
Fortran-ordered, i.e. breeze's column-major DenseMatrix (S/fm/FMModel.scala:19) — and a
device-resident fp32 twin behind the C ABI.  Host and device copies are synchronised lazily.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .dataset import DataSet
from .relational import RelationalData


class Model:
    """S/Model.scala:9-32."""

    def predict(self, features):
        raise NotImplementedError

    def computeRMSE(self, dataset):
        raise NotImplementedError

    # The remaining metrics of S/Model.scala are off the training path and buggy in the reference
    # (quirk Q4): computeMAE there is a SIGNED mean error (no abs, :21-26) and computeAccuracy does
    # an integer division that yields 0 or 1 (:28-30).  Here they are what their names say; the
    # reference's signed quantity is available as computeMeanError.
    def computeMeanError(self, dataset):
        """mean of (target - prediction): what the reference's `computeMAE` actually returns."""
        return float((dataset.y - self.predict(dataset)).mean()) if dataset.size else 0.0

    def computeMAE(self, dataset):
        return float(abs(dataset.y - self.predict(dataset)).mean()) if dataset.size else 0.0

    def computeAccuracy(self, dataset):
        """fraction of rows whose prediction has the target's sign (>= 0 vs < 0), S/Model.scala:29."""
        if not dataset.size:
            return 0.0
        yh = self.predict(dataset)
        return float((((dataset.y >= 0) & (yh >= 0)) | ((dataset.y < 0) & (yh < 0))).mean())


class FMModel(Model):
    def __init__(self, num_attribute, num_factor, init_mean=0.0, init_stdev=0.01, seed=0, device=0, stream=None,
                 init_on_device=False):
        self.num_attribute = int(num_attribute)  # S/fm/FMModel.scala:10
        self.num_factor = int(num_factor)
        self.init_mean, self.init_stdev, self.seed = init_mean, init_stdev, seed
        n1 = self.num_attribute + 1
        # S/fm/FMModel.scala:17-22: w0 = 0, w = 0, v ~ N(mean, stdev).  The reference ignores `seed`
        # (quirk Q2: unseeded breeze Gaussian); here the seed IS honoured so runs are reproducible.
        # init_on_device: the draw happens on the GPU (fmhip_model_init_normal) and no host copy exists until
        # one is asked for — for models too wide to stage on the host (2^25 x 64 doubles = 17 GB)
        self._init_on_device = bool(init_on_device)
        self._w0 = 0.0
        self._w = np.zeros(n1)
        if self._init_on_device:
            self._v = None
        else:
            rng = np.random.Generator(np.random.PCG64(seed))
            self._v = np.asfortranarray(rng.normal(init_mean, init_stdev, size=(n1, self.num_factor)).T)
        self.k0 = True  # S/fm/FMModel.scala:25-26
        self.k1 = True
        self.reg0, self.regw, self.regv = 0.0, 0.0, 10.0  # S/fm/FMModel.scala:29-31 (ALS ridge terms)
        self.device = int(device)
        self._stream = stream
        self._h = None
        self._host_fresh = not self._init_on_device   # host arrays hold the current parameters
        self._dev_fresh = False                       # device holds the current parameters
        self._lost = False                            # close() dropped the only copy of the parameters (see close)

    # -- parameter access (lazy host<->device sync) --------------------------------------
    def _pull(self):
        if self._lost:
            raise RuntimeError("this FMModel's parameters were discarded by close(): the device copy was freed without being read back "
                               "(close(discard=True), or a model drawn on the device that nobody had read) — pull them before closing "
                               "(fm.v, fm.rows(ids)) or assign new ones (fm.w0, fm.w, fm.v = ...)")
        if not self._host_fresh:
            w0 = C.c_double()
            flat = np.empty(self.num_factor * (self.num_attribute + 1))
            _ffi.check(_ffi.load().fmhip_model_get_params(self.handle, C.byref(w0), _ffi.ptr(self._w), _ffi.ptr(flat)))
            self._w0 = w0.value
            self._v = flat.reshape((self.num_factor, self.num_attribute + 1), order="F")
            self._host_fresh = True

    @property
    def w0(self):
        self._pull()
        return self._w0

    def _assign(self):
        """Before a setter replaces one of the three parameters: the other two must be current (or, after a discarding
        close, restart from the state of a fresh model so that assigning all three brings the model back)."""
        if self._lost:
            self._lost = False
            self._host_fresh = True
            self._w0 = 0.0
            self._w = np.zeros(self.num_attribute + 1)
            self._v = np.zeros((self.num_factor, self.num_attribute + 1), order="F")
        self._pull()

    @w0.setter
    def w0(self, x):
        self._assign()
        self._w0 = float(x)
        self._dev_fresh = False

    @property
    def w(self):
        """Mutating the returned array in place requires a following ``touch()``."""
        self._pull()
        return self._w

    @w.setter
    def w(self, x):
        self._assign()
        self._w = np.array(x, np.float64).reshape(self.num_attribute + 1)
        self._dev_fresh = False

    @property
    def v(self):
        self._pull()
        return self._v

    @v.setter
    def v(self, x):
        self._assign()
        x = np.asarray(x, np.float64)
        if x.shape != (self.num_factor, self.num_attribute + 1):
            raise ValueError("v must have shape (num_factor, num_attribute + 1)")
        self._v = np.asfortranarray(x)
        self._dev_fresh = False

    def rows(self, ids):
        """(w[ids], v[:, ids]) straight from the device — `fm.w(i)`, `fm.v(::, i)` of the reference for a few features,
        without copying a model that may not fit the host (fmhip_model_get_rows)."""
        ids = np.ascontiguousarray(ids, np.int32)
        w = np.empty(len(ids))
        v = np.empty(len(ids) * self.num_factor)
        _ffi.check(_ffi.load().fmhip_model_get_rows(self.handle, len(ids), _ffi.ptr(ids), _ffi.ptr(w), _ffi.ptr(v)))
        return w, v.reshape((self.num_factor, len(ids)), order="F")

    def touch(self):
        """Declare that the host arrays were modified in place."""
        self._pull()
        self._dev_fresh = False

    @property
    def handle(self):
        """Device model with the current parameters uploaded."""
        L = _ffi.load()
        if self._lost:
            self._pull()       # raises: there is nothing to upload
        if self._h is None:
            h = C.c_void_p()
            _ffi.check(L.fmhip_model_create(self.device, self.num_attribute, self.num_factor, self._stream, C.byref(h)))
            self._h = h
            if self._init_on_device and not self._host_fresh:
                _ffi.check(L.fmhip_model_init_normal(h, self.seed, self.init_mean, self.init_stdev))
                self._dev_fresh = True
        if not self._dev_fresh:
            flat = np.ascontiguousarray(self._v.reshape(-1, order="F"))
            _ffi.check(L.fmhip_model_set_params(self._h, self._w0, _ffi.ptr(self._w), _ffi.ptr(flat)))
            self._dev_fresh = True
        return self._h

    def _device_updated(self):
        self._host_fresh = False
        self._dev_fresh = True

    def close(self, discard=False):
        """Frees the device model.  The parameters are copied back to the host first so that `fm.w` / `fm.v` keep
        working — except with `discard=True`, or for a model drawn on the device (`init_on_device=True`: it exists so
        that no host copy is made until one is asked for; at 2^25 x 64 the copy is 8.6 GB of fp32 staging plus a 17 GB
        fp64 array) whose parameters nobody has read yet.  After such a close the trained values are GONE and the model
        says so: `fm.w` / `fm.v` / `predict` raise until new parameters are assigned — it does not quietly hand back stale
        host arrays or re-draw the initial ones.  Pull them first (`fm.v`, `fm.rows(ids)`) if they are wanted."""
        if self._h is not None:
            if not discard and not (self._init_on_device and self._v is None):
                self._pull()
            elif not self._host_fresh:
                self._lost = True          # the device held the only current copy
            _ffi.load().fmhip_model_destroy(self._h)
            self._h = None
            self._dev_fresh = False

    def __del__(self):
        try:
            if self._h is not None:
                _ffi.load().fmhip_model_destroy(self._h)
        except Exception:
            pass

    # -- scoring -------------------------------------------------------------------------
    def predict(self, features):
        """FMModel.predict (S/fm/FMModel.scala:34-55).  `features` is one sparse row
        ``(indices, values)`` -> float, or a DataSet -> array (the rdd.mapValues(predict) of
        S/Model.scala:14)."""
        if isinstance(features, RelationalData):        # every block's forward once, then one combine per data row
            out = np.empty(features.size)
            _ffi.check(_ffi.load().fmhip_relational_predict(self.handle, features.rel_handle, _ffi.ptr(out)))
            return out
        if isinstance(features, DataSet):
            out = np.empty(features.size)
            _ffi.check(_ffi.load().fmhip_predict(self.handle, features.handle, _ffi.ptr(out)))
            return out
        idx, val = features
        idx = np.ascontiguousarray(idx, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        if len(idx) != len(val):
            raise ValueError("index/value length mismatch")
        out = np.empty(1)
        _ffi.check(_ffi.load().fmhip_predict_rows(self.handle, 1, _ffi.ptr(np.array([0, len(idx)], np.int64)), _ffi.ptr(idx),
                                                  _ffi.ptr(val), _ffi.ptr(out)))
        return float(out[0])

    def computeRMSE(self, dataset):
        """Model.computeRMSE (S/Model.scala:13-19)."""
        r = C.c_double()
        if isinstance(dataset, RelationalData):
            _ffi.check(_ffi.load().fmhip_relational_rmse(self.handle, dataset.rel_handle, C.byref(r), None))
            return r.value
        _ffi.check(_ffi.load().fmhip_rmse(self.handle, dataset.handle, C.byref(r), None))
        return r.value

    def computeLogLoss(self, dataset):
        """Mean log-loss of sigmoid(predict) against the labels t = [y > 0], whatever loss the model was trained
        under (fmhip_logloss; binary classification — the reference declares Task.Classification and scores it only by
        sign, S/Model.scala:28-30)."""
        r = C.c_double()
        if isinstance(dataset, RelationalData):
            _ffi.check(_ffi.load().fmhip_relational_logloss(self.handle, dataset.rel_handle, C.byref(r), None))
            return r.value
        _ffi.check(_ffi.load().fmhip_logloss(self.handle, dataset.handle, C.byref(r), None))
        return r.value

    def weightedScores(self, dataset):
        """The weighted scores of the predictions over a weighted dataset (``DataSet(..., weights=)``; fmhip_weighted_scores): a
        dict of sum_w, rmse = sqrt(sum c (yhat - y)^2 / sum c), mae, logloss (the weighted mean of computeLogLoss's row terms), rows,
        nonfinite.  nan ratios when the weights sum to 0; an unweighted dataset is refused."""
        res = _ffi.WeightedResult()
        _ffi.check(_ffi.load().fmhip_weighted_scores(self.handle, dataset.handle, C.byref(res)))
        return res.as_dict()

    def computeWeightedRMSE(self, dataset):
        """sqrt(sum c (predict - y)^2 / sum c) over a weighted dataset; computeRMSE ignores the weights."""
        return self.weightedScores(dataset)["rmse"]

    def computeWeightedLogLoss(self, dataset):
        """Weighted mean log-loss over a weighted dataset — on a test set with down-sampled negatives weighted back up, the
        log-loss of the traffic; computeLogLoss ignores the weights."""
        return self.weightedScores(dataset)["logloss"]

    def _pair_score(self, dataset):
        r, c = C.c_double(), C.c_double()
        _ffi.check(_ffi.load().fmhip_pair_logloss(self.handle, dataset.handle, C.byref(r), C.byref(c), None))
        return r.value, c.value

    def computePairLogLoss(self, dataset):
        """Mean pairwise log-loss over the pairs (rows 2j, 2j+1) of `dataset` (``DataSet.from_pairs``): -log sigmoid(d) of the
        margin d = predict(row 2j) - predict(row 2j+1) when row 2j carries the larger label, -log sigmoid(-d) otherwise
        (fmhip_pair_logloss); log 2 for a model that cannot tell the rows apart."""
        return self._pair_score(dataset)[0]

    def computePairAccuracy(self, dataset):
        """Share of the pairs of `dataset` the model orders as their labels do (a tie counts one half): the pairwise AUC
        (fmhip_pair_logloss's concordance)."""
        return self._pair_score(dataset)[1]

    def aucDetails(self, dataset, groups=None, stats=False):
        """Every field of fmhip_auc's result as a dict — u2, pairs, positives, negatives, groups, groups_scored, auc, gauc (and,
        with stats=True, "stats": what computeRMSE's pass reports) — for the model's predictions on `dataset` against the labels
        t = [y > 0].  `groups`: None (one group), or one integer id in [0, 2^31) per row — only pairs of rows that share an id
        count.  Ranked on the device as the fp32 values `predict` returns, exactly: -0 ties with +0, NaN ranks below -inf."""
        res, st = _ffi.AucResult(), _ffi.Stats()
        g = _ffi.group_ids(groups, dataset.size)
        _ffi.check(_ffi.load().fmhip_auc(self.handle, dataset.handle, _ffi.ptr(g), C.byref(res), C.byref(st) if stats else None))
        out = res.as_dict()
        if stats:
            out["stats"] = st.as_dict()
        return out

    def computeAUC(self, dataset, groups=None):
        """Area under the ROC curve of the model's predictions on `dataset` (fmhip_auc): the share of (positive, negative) pairs
        the model orders correctly, a tie counting one half; with `groups`, over the pairs inside a group only.  nan when there
        is no such pair."""
        return self.aucDetails(dataset, groups)["auc"]

    def computeGroupAUC(self, dataset, groups):
        """GAUC: the AUC inside each group (a user's impressions) averaged by the groups' row counts, over the groups that hold
        both classes; nan when there is none."""
        return self.aucDetails(dataset, groups)["gauc"]

    def residual(self, dataset):
        """ALS.precomputeTermE (S/fm/lib/ALS.scala:142-144): e = predict - target."""
        out = np.empty(dataset.size)
        _ffi.check(_ffi.load().fmhip_residual(self.handle, dataset.handle, _ffi.ptr(out)))
        return out

    def termQ(self, dataset):
        """ALS.precomputeTermQ for all factors (S/fm/lib/ALS.scala:146-150): (rows, k)."""
        out = np.empty((dataset.size, self.num_factor))
        _ffi.check(_ffi.load().fmhip_term_q(self.handle, dataset.handle, _ffi.ptr(out)))
        return out

    def recommend(self, contexts, candidates, k, exclude=None, scores=True):
        """Per row of `contexts` the `k` rows of `candidates` the model ranks highest (fmhip_topk): the score of a pair is
        FMModel.predict (S/fm/FMModel.scala:34) of the row "the context's entries, then the candidate's" — the users x items
        ranking the reference's demo trains for (S/driver.scala:100-112) — without ever forming the joined rows or the full
        score matrix.  -> (idx int32 [B, k], score float64 [B, k]) (score is None with scores=False); best first, equal scores by
        ascending candidate row, NaN last; fewer than k candidates left: -1 / -inf.  `exclude`: None, or one integer array of
        candidate rows per context that must not be returned (sorted and de-duplicated here)."""
        B, k = contexts.size, int(k)
        if not 1 <= k <= _ffi.TOPK_MAX:
            raise ValueError("k must be in [1, %d], not %d" % (_ffi.TOPK_MAX, k))
        eptr = eidx = None
        if exclude is not None:
            eptr, eidx = _ffi.row_lists(exclude, B, candidates.size, "exclude")
        idx = np.empty((B, k), np.int32)
        score = np.empty((B, k)) if scores else None
        _ffi.check(_ffi.load().fmhip_topk(self.handle, contexts.handle, candidates.handle, k, _ffi.ptr(eptr), _ffi.ptr(eidx),
                                          _ffi.ptr(idx), _ffi.ptr(score)))
        return idx, score

    def pairScores(self, contexts, candidates, c0=0, c1=None):
        """The scores `recommend` ranks by, in full, for the contexts [c0, c1) (fmhip_pair_scores): [c1 - c0, candidates.size]."""
        c0, c1 = int(c0), contexts.size if c1 is None else int(c1)
        if not 0 <= c0 <= c1 <= contexts.size:
            raise ValueError("contexts [%d, %d) outside [0, %d]" % (c0, c1, contexts.size))
        out = np.empty((c1 - c0, candidates.size))
        _ffi.check(_ffi.load().fmhip_pair_scores(self.handle, contexts.handle, candidates.handle, c0, c1, _ffi.ptr(out)))
        return out

    def rankOf(self, contexts, candidates, relevant, exclude=None, scores=False):
        """Where the model ranks given candidates (fmhip_rank): `relevant` holds one integer array of candidate rows per context
        (sorted and de-duplicated here, as `exclude`); -> one int32 array per context, the 0-based position of each of those rows,
        ascending by row, in the context's COMPLETE ranking — what `recommend` would return with k = candidates.size: best
        first, equal scores by ascending row, NaN last — counted on the device from the bits `pairScores` returns, without
        forming the scores.  `exclude`: None, or per context the candidate rows that are not in the ranking (what the user
        rated in training); a row both relevant and excluded for a context raises ValueError.  scores=True: -> (ranks, scores),
        the score of every relevant row beside its rank."""
        B, M = contexts.size, max(candidates.size, 1)
        rptr, ridx = _ffi.row_lists(relevant, B, candidates.size, "relevant")
        n = int(rptr[B])
        eptr = eidx = None
        if exclude is not None:
            eptr, eidx = _ffi.row_lists(exclude, B, candidates.size, "exclude")
            # (context, row) words of the exclusions ascend: one binary search per relevant row
            ctx_of = lambda ptr: np.repeat(np.arange(B, dtype=np.int64), np.diff(ptr))       # noqa: E731
            ekey, rkey = ctx_of(eptr) * M + eidx[:int(eptr[B])], ctx_of(rptr) * M + ridx[:n]
            at = np.minimum(np.searchsorted(ekey, rkey), max(len(ekey) - 1, 0))
            both = rkey[ekey[at] == rkey] if len(ekey) else rkey[:0]
            if len(both):
                raise ValueError("candidate row %d is both relevant and excluded for context %d" % (both[0] % M, both[0] // M))
        rank = np.empty(max(n, 1), np.int32)
        score = np.empty(max(n, 1)) if scores else None
        _ffi.check(_ffi.load().fmhip_rank(self.handle, contexts.handle, candidates.handle, _ffi.ptr(rptr), _ffi.ptr(ridx),
                                          _ffi.ptr(eptr), _ffi.ptr(eidx), _ffi.ptr(rank), _ffi.ptr(score)))
        ranks = [rank[rptr[c]:rptr[c + 1]] for c in range(B)]
        if not scores:
            return ranks
        return ranks, [score[rptr[c]:rptr[c + 1]] for c in range(B)]

    def computeRankingMetrics(self, contexts, candidates, relevant, k=10, exclude=None):
        """HitRate@k, Recall@k, Precision@k, NDCG@k, MRR and MAP of the relevant rows' ranks (`rankOf`, then fmhip_rank_metrics on
        the host), averaged over the contexts that have a relevant row: a dict of k, contexts, skipped, relevant, hit_rate,
        recall, precision, ndcg, mrr, map."""
        from . import metrics
        if int(k) < 1:
            raise ValueError("k must be >= 1, not %d" % int(k))
        return metrics.ranking_metrics(self.rankOf(contexts, candidates, relevant, exclude=exclude), k)

    def batchGradient(self, dataset, batch=0):
        """sum over the batch of e*h (h: S/fm/lib/ALS.scala:56-58,40,21) -> (gv (k,n1), gw, g0, stats)."""
        n1 = self.num_attribute + 1
        gv = np.empty(self.num_factor * n1)
        gw = np.empty(n1)
        g0 = C.c_double()
        st = _ffi.Stats()
        _ffi.check(_ffi.load().fmhip_batch_grad(self.handle, dataset.handle, batch, _ffi.ptr(gv), _ffi.ptr(gw),
                                                C.byref(g0), C.byref(st)))
        return gv.reshape((self.num_factor, n1), order="F"), gw, g0.value, st.as_dict()

    # -- FTRL-Proximal (include/fmhip_ftrl.h) --------------------------------------------
    def nonzeros(self):
        """Exact counts over the model on the device (fmhip_model_nonzeros): dict of w_nonzero (of w_total = num_attribute + 1),
        v_nonzero (of v_total = w_total * num_factor) and features_all_zero — features whose w and whole V row are zero."""
        w, v, z = C.c_int64(), C.c_int64(), C.c_int64()
        _ffi.check(_ffi.load().fmhip_model_nonzeros(self.handle, C.byref(w), C.byref(v), C.byref(z)))
        n1 = self.num_attribute + 1
        return dict(w_nonzero=int(w.value), v_nonzero=int(v.value), features_all_zero=int(z.value), w_total=n1,
                    v_total=n1 * self.num_factor)

    def ftrl_state(self):
        """The FTRL state of a model under that rule (``HipFTRL``; fmhip_model_get_ftrl_state), for checkpoints: dict of z0, zw
        (n1), zv (k, n1), n0, nw, nv — zeta and n of w0, w and v, shaped like them."""
        n1, k = self.num_attribute + 1, self.num_factor
        z0, n0 = C.c_double(), C.c_double()
        zw, nw, zv, nv = np.empty(n1), np.empty(n1), np.empty(k * n1), np.empty(k * n1)
        _ffi.check(_ffi.load().fmhip_model_get_ftrl_state(self.handle, C.byref(z0), _ffi.ptr(zw), _ffi.ptr(zv), C.byref(n0),
                                                          _ffi.ptr(nw), _ffi.ptr(nv)))
        return dict(z0=z0.value, zw=zw, zv=zv.reshape((k, n1), order="F"), n0=n0.value, nw=nw, nv=nv.reshape((k, n1), order="F"))

    def set_ftrl_state(self, state):
        """Writes a state read by ``ftrl_state`` back (fmhip_model_set_ftrl_state).  The model must be under FTRL with the settings
        the state was trained with (``_ffi.FtrlRule(...).set_on(fm.handle)``, or a first ``HipFTRL`` step): parameters and state
        restored into a fresh model continue the run bit for bit."""
        n1, k = self.num_attribute + 1, self.num_factor
        flat = {}
        for name, shape in (("zw", (n1,)), ("nw", (n1,)), ("zv", (k, n1)), ("nv", (k, n1))):
            a = np.asarray(state[name], np.float64)
            if a.shape != shape:
                raise ValueError("%s must have shape %r, not %r" % (name, shape, a.shape))
            flat[name] = np.ascontiguousarray(a.reshape(-1, order="F"))
        _ffi.check(_ffi.load().fmhip_model_set_ftrl_state(self.handle, float(state["z0"]), _ffi.ptr(flat["zw"]), _ffi.ptr(flat["zv"]),
                                                          float(state["n0"]), _ffi.ptr(flat["nw"]), _ffi.ptr(flat["nv"])))
