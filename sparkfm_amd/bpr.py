"""HipBPR — BPR on implicit feedback over a block of contexts and a block of candidates (include/fmhip_bpr.h).

``HipSGD.run(loss="logistic", pairs=True)`` trains BPR on a flat ``DataSet.from_pairs(preferred, other)`` whose `other` rows the
caller has to choose, join and rebuild every epoch.  ``HipBPR`` takes what ``FMModel.recommend`` takes — the users once, the items
once — and the observed interactions as one array of candidate rows per context (the format of ``exclude=``); the negatives are
drawn on the device afresh for every epoch and the step is the relational one, so nothing joined is ever built:

    bpr = HipBPR.run(users, items, positives, n_neg=1, eta=0.05, regv=0.01)
    fm = bpr.fit(k=16, epochs=20)                          # or FM(users, 16, maxIteration=20).learnWith(bpr)
    fm.computeRankingMetrics(users, items, held_out, exclude=positives)
"""
import ctypes as C
import operator

import numpy as np

from . import _ffi
from .dataset import DataSet
from .learn import FMLearn
from .model import FMModel


class HipBPR(FMLearn):
    """One ``learn`` = one epoch at t = the epochs done: the negatives redrawn, then every batch (redraw="epoch"), or every batch's
    negatives redrawn right before its step under the model as it then stands (redraw="batch", include/fmhip_redraw.h).

    `contexts`, `candidates`: single-batch training ``DataSet``s (batch_rows=0, not scoring-only, unweighted; labels unused) with
    disjoint feature ids.  `positives`: one integer array of candidate rows per context (sorted and de-duplicated here).  There are
    n_pairs = n_neg * (number of interactions) pairs; pair p belongs to interaction p // n_neg of the TRAINING ORDER, fixed here:
    context-ascending (rows ascending inside a context), or with shuffle=True a ``PCG64([seed])`` permutation of that.
    `batch_pairs`: pairs per mini-batch (0: one batch).  `seed` also keys the sampler.  `loss`: "logistic" (BPR) or "squared" (the
    squared pair loss); `optimizer` and the AdaGrad settings as ``HipSGD``.  The model's pairing flag is neither read nor set.
    `n_candidates` (1 .. 64): above 1 every epoch draws that many candidates per pair and trains on the one the model scores
    highest (include/fmhip_bpr_adaptive.h) — at the epoch's start under redraw="epoch", at the batch's own step under
    redraw="batch"; 1 is the uniform sampler, bit for bit what it was.
    `sampler`: "auto" (that: uniform at n_candidates = 1, the best of n_candidates above) or "warp" (include/fmhip_warp.h): every
    epoch keeps per pair the FIRST of its n_candidates candidates whose score is above the positive's minus `margin` (>= 0), and
    the step trains a hinge at that margin weighted by the rank estimated from how many candidates that took; pairs without a
    violator get weight 0.  With "warp" `loss` stays at its default — the hinge takes its place and the model's loss is not set.
    `redraw`: "epoch" (one draw of every pair per ``learn``, one synchronisation for it) or "batch" (include/fmhip_redraw.h): batch
    b's pairs are drawn between batch b's forwards and the rest of its step, the candidate rows being those of the per-epoch draw
    and the scores — hence the choice, and WARP's weights — the current model's; an epoch still synchronises once, at its end.  A
    uniform sampler trains the same bits in both modes.
    `negatives`: the proposal every candidate row is drawn from (include/fmhip_proposal.h) — "uniform" (the default: bit for bit what
    it was), "popularity" (row i in proportion to (n_i + smooth) ** power, n_i the number of contexts whose positives list row i;
    power = 0.75 is word2vec's noise distribution; `smooth` > 0 keeps every row drawable) or an array of M finite weights > 0.  It
    composes with every sampler and both redraws: the n_candidates candidates of the best-of and WARP rules come from it too.
    WARP's rank estimate stays (M - 1) // N.  A fresh handle holds the uniform draw at t = 0 until its first resample or learn.
    `loss="softmax"` (include/fmhip_softmax.h): the n_neg negatives of an interaction compete in one sampled-softmax loss,
    -log softmax(s+ | s+, s-_1 .. s-_n), instead of forming n_neg independent pairs; at n_neg = 1 it is logistic BPR.  The trainer
    handles it itself — the model's loss is neither read nor set.  It composes with n_candidates, both redraws and `negatives`, not
    with sampler="warp"; `batch_pairs` must be a multiple of n_neg.  `logq=True` subtracts the proposal's log-probabilities from the
    logits (the log-Q correction of a sampled softmax); it is ignored under the uniform proposal."""

    SAMPLERS = ("auto", "warp")
    REDRAWS = ("epoch", "batch")
    NEGATIVES = ("uniform", "popularity")

    def __init__(self, contexts, candidates, positives, n_neg=1, batch_pairs=0, seed=0, shuffle=True, eta=0.05, reg0=0.0, regw=0.0,
                 regv=0.0, loss="logistic", optimizer="sgd", adagrad_eps=1e-10, adagrad_init=0.1, n_candidates=1, sampler="auto", margin=1.0,
                 redraw="epoch", negatives="uniform", power=0.75, smooth=1.0, logq=False):
        for what, d in (("contexts", contexts), ("candidates", candidates)):
            if not isinstance(d, DataSet):
                raise TypeError("%s must be a DataSet, not %s" % (what, type(d).__name__))
            if d.scoring:
                raise ValueError("%s is a scoring-only DataSet: the trainer needs its transposes (make it without scoring=True)" % what)
            if d.weights is not None:
                raise ValueError("%s carries example weights: the BPR trainer takes unweighted blocks" % what)
            if 0 < d.batch_rows < d.size:
                raise ValueError("%s has more than one batch: make it with batch_rows=0" % what)
        if contexts.device != candidates.device:
            raise ValueError("contexts on device %d, candidates on device %d" % (contexts.device, candidates.device))
        self.n_neg = operator.index(n_neg)
        if self.n_neg < 1:
            raise ValueError("n_neg must be >= 1, not %d" % self.n_neg)
        if candidates.size < 2:
            raise ValueError("candidates has %d rows: a pair needs at least 2" % candidates.size)
        if isinstance(n_candidates, bool):
            raise TypeError("n_candidates must be an integer, not %r" % (n_candidates,))
        self._n_candidates = operator.index(n_candidates)
        if not 1 <= self._n_candidates <= _ffi.BPR_MAX_CANDIDATES:
            raise ValueError("n_candidates must be in [1, %d], not %d" % (_ffi.BPR_MAX_CANDIDATES, self._n_candidates))
        if sampler not in self.SAMPLERS:
            raise ValueError("sampler must be one of %s, not %r" % (", ".join(repr(s) for s in self.SAMPLERS), sampler))
        self._sampler = sampler
        if not isinstance(redraw, str) or redraw not in self.REDRAWS:
            raise ValueError("redraw must be one of %s, not %r" % (", ".join(repr(s) for s in self.REDRAWS), redraw))
        self._redraw = redraw
        if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) \
                or not 0 <= float(margin) <= float(np.finfo(np.float32).max):      # (the device's margin is fp32; a NaN fails both)
            raise ValueError("margin must be a finite number >= 0, not %r" % (margin,))
        self._margin = float(margin)
        self._softmax = isinstance(loss, str) and loss == "softmax"
        if not isinstance(logq, (bool, np.bool_)):
            raise ValueError("logq must be True or False, not %r" % (logq,))
        self._logq = bool(logq)
        if sampler == "warp" and self._softmax:
            raise ValueError("sampler='warp' trains its own hinge and loss='softmax' its own rule: choose one of them")
        if sampler == "warp" and loss != "logistic":
            raise ValueError("sampler='warp' trains its own hinge: leave loss at its default, not %r" % (loss,))
        self.seed = operator.index(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64), not %r" % (seed,))
        if not isinstance(shuffle, bool):
            raise ValueError("shuffle must be True or False, not %r" % (shuffle,))
        self.contexts, self.candidates = contexts, candidates
        ptr, rows = _ffi.row_lists(positives, contexts.size, candidates.size, "positives")
        n = int(ptr[-1])
        if n < 1:
            raise ValueError("positives holds no interaction")
        full = np.flatnonzero(np.diff(ptr) >= candidates.size)
        if len(full):
            raise ValueError("context %d has all %d candidate rows as positives: no negative exists for it" % (full[0], candidates.size))
        if 2 * n * self.n_neg >= 2 ** 31:
            raise ValueError("n_neg * interactions = %d pairs: 2 * n_pairs must stay below 2^31" % (n * self.n_neg))
        self.positives_ptr, self.positives_rows = ptr, rows[:n].copy()
        ictx = np.repeat(np.arange(contexts.size, dtype=np.int32), np.diff(ptr))
        icand = self.positives_rows
        if shuffle:
            perm = np.random.Generator(np.random.PCG64([self.seed])).permutation(n)
            ictx, icand = ictx[perm], icand[perm]
        self.inter_ctx, self.inter_cand = np.ascontiguousarray(ictx, np.int32), np.ascontiguousarray(icand, np.int32)
        self.n_pairs = n * self.n_neg
        bp = operator.index(batch_pairs)
        self.batch_pairs = bp if 0 < bp <= self.n_pairs else self.n_pairs
        if self._softmax and self.batch_pairs < self.n_pairs and self.batch_pairs % self.n_neg:
            raise ValueError("loss='softmax': batch_pairs = %d is no multiple of n_neg = %d — a batch would split an interaction's negatives"
                             % (self.batch_pairs, self.n_neg))
        self.shuffle = shuffle
        self.eta, self.reg0, self.regw, self.regv = float(eta), float(reg0), float(regw), float(regv)
        self.loss, self.optimizer = loss, optimizer
        self._loss_code = None if self._softmax else _ffi.loss_code(loss)      # (the softmax is the trainer's own rule, not a model loss)
        self._opt_code = _ffi.optimizer_code(optimizer)
        self.adagrad_eps, self.adagrad_init = _ffi.adagrad_settings(adagrad_eps, adagrad_init)
        self.device = contexts.device
        self._h, self._for = None, None
        self._epoch = 0
        self.last_stats = None
        self.sample_stats = None
        self._proposal = None
        if isinstance(negatives, str):
            if negatives not in self.NEGATIVES:
                raise ValueError("negatives must be one of %s, or an array of %d weights, not %r"
                                 % (", ".join(repr(s) for s in self.NEGATIVES), candidates.size, negatives))
            if negatives == "popularity":
                self._proposal = self._checked_weights(self.popularity_weights(power, smooth))
        else:
            self._proposal = self._checked_weights(negatives)

    def popularity_weights(self, power=0.75, smooth=1.0):
        """float64 [M]: (n_i + smooth) ** power, n_i the number of contexts whose positives list row i."""
        for what, x in (("power", power), ("smooth", smooth)):
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
                raise ValueError("%s must be a finite number, not %r" % (what, x))
        if not smooth > 0:
            raise ValueError("smooth must be > 0 (every row needs a positive weight), not %r" % (smooth,))
        counts = np.bincount(self.positives_rows, minlength=self.candidates.size).astype(np.float64)
        return (counts + float(smooth)) ** float(power)

    def _checked_weights(self, weights):
        """A copy of `weights` as float64 [M], every entry finite and > 0; ValueError otherwise."""
        if weights is None or isinstance(weights, (str, bytes)):
            raise ValueError("negatives must be 'uniform', 'popularity' or an array of %d weights, not %r" % (self.candidates.size, weights))
        w = np.array(weights, np.float64)
        if w.shape != (self.candidates.size,):
            raise ValueError("the proposal takes one weight per candidate row: shape (%d,), not %r" % (self.candidates.size, w.shape))
        bad = np.flatnonzero(~(np.isfinite(w) & (w > 0)))
        if len(bad):
            raise ValueError("weights[%d] = %r: a proposal weight is finite and > 0" % (bad[0], float(w[bad[0]])))
        if not np.isfinite(sum(w.tolist())):
            raise ValueError("the sum of the weights is not finite")
        w.setflags(write=False)
        return w

    @classmethod
    def run(cls, contexts, candidates, positives, **kw):
        return cls(contexts, candidates, positives, **kw)

    # -- what the fit loop reads ------------------------------------------------------------
    @property
    def dimension(self):
        """The larger of the two blocks' dimensions: what a model that trains on them must hold."""
        return max(self.contexts.dimension, self.candidates.dimension)

    @property
    def n_batches(self):
        return (self.n_pairs + self.batch_pairs - 1) // self.batch_pairs

    @property
    def handle(self):
        """The trainer's handle.  It borrows the two blocks' device copies: when either has been unpersisted since (``learnWith``
        unpersists its dataset argument), the handle is made again over the fresh copies — the draw is then the one at t = 0."""
        blocks = (self.contexts.cache()._h, self.candidates.cache()._h)
        if self._h is not None and (self._for[0] is not blocks[0] or self._for[1] is not blocks[1]):
            self.close()
        if self._h is None:
            h = C.c_void_p()
            _ffi.check(_ffi.load().fmhip_bpr_create(self.device, blocks[0], blocks[1], len(self.inter_ctx), _ffi.ptr(self.inter_ctx),
                                                    _ffi.ptr(self.inter_cand), self.n_neg, self.batch_pairs, self.seed, C.byref(h)))
            self._h, self._for = h, blocks
            if self._n_candidates > 1:
                _ffi.check(_ffi.load().fmhip_bpr_set_candidates(h, self._n_candidates))
            if self.warp:
                _ffi.check(_ffi.load().fmhip_warp_set(h, 1, self._margin))
            if self._redraw != "epoch":
                _ffi.check(_ffi.load().fmhip_redraw_set(h, _ffi.REDRAWS[self._redraw]))
            if self._proposal is not None:
                _ffi.check(_ffi.load().fmhip_proposal_set(h, _ffi.ptr(self._proposal)))
            if self._softmax:
                _ffi.check(_ffi.load().fmhip_softmax_set(h, 1, int(self._logq)))
        return self._h

    @property
    def proposal(self):
        """None under the uniform proposal, else the float64 [M] weights the candidate rows are drawn in proportion to."""
        return self._proposal

    def set_proposal(self, weights):
        """The proposal from the next draw on (fmhip_proposal_set): None for uniform, or M finite weights > 0.  The standing draw is
        left as it is.  A refusal leaves the proposal that was in force."""
        w = None if weights is None else self._checked_weights(weights)
        if self._h is not None:
            _ffi.check(_ffi.load().fmhip_proposal_set(self._h, _ffi.ptr(w)))
        self._proposal = w

    def proposal_table(self):
        """(thresh uint32 [M], alias int32 [M]): the alias table the device draws from (fmhip_proposal_table); the proposal must
        be a weighted one."""
        if self._proposal is None:
            raise ValueError("the proposal is uniform: it has no table")
        thresh, alias = np.empty(self.candidates.size, np.uint32), np.empty(self.candidates.size, np.int32)
        _ffi.check(_ffi.load().fmhip_proposal_table(self.handle, _ffi.ptr(thresh), _ffi.ptr(alias)))
        return thresh, alias

    @property
    def n_candidates(self):
        """Candidates drawn per pair and epoch (include/fmhip_bpr_adaptive.h); 1: the uniform sampler."""
        return self._n_candidates

    @property
    def sampler(self):
        return self._sampler

    @property
    def redraw(self):
        """"epoch" or "batch": when ``learn`` redraws the negatives (include/fmhip_redraw.h)."""
        return self._redraw

    @property
    def margin(self):
        """The WARP margin (read only with sampler="warp")."""
        return self._margin

    @property
    def warp(self):
        return self._sampler == "warp"

    def info(self):
        v = [C.c_int64() for _ in range(4)]
        m = C.c_int32()
        _ffi.check(_ffi.load().fmhip_bpr_info(self.handle, *[C.byref(x) for x in v], C.byref(m)))
        return dict(zip(("n_pairs", "dimension", "batch_pairs", "n_batches", "n_neg"), [int(x.value) for x in v] + [int(m.value)]))

    def close(self):
        """Frees the handle (the blocks stay cached: they are the caller's)."""
        if self._h is not None:
            _ffi.load().fmhip_bpr_destroy(self._h)
            self._h, self._for = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the draw ---------------------------------------------------------------------------
    def resample(self, t, fm=None):
        """Redraws every pair's negative at epoch `t` -> ``sample_stats``.  Without a model the draw is uniform (fmhip_bpr_resample:
        attempts, forced).  With `fm` it is the best of `n_candidates` candidates under the model as it stands
        (fmhip_bpr_resample_adaptive: attempts, forced, replaced — the pairs whose kept candidate is not the uniform draw).
        With sampler="warp" it is the WARP draw under `fm` (fmhip_warp_resample: pairs, violated, trials), and a model is required."""
        if self.warp:
            if fm is None:
                raise ValueError("sampler='warp': the WARP draw needs a model — resample(t, fm)")
            st = _ffi.WarpStats()
            _ffi.check(_ffi.load().fmhip_warp_resample(fm.handle, self.handle, operator.index(t), C.byref(st)))
        elif fm is None:
            if self._n_candidates > 1:
                raise ValueError("n_candidates = %d: the adaptive draw needs a model — resample(t, fm)" % self._n_candidates)
            st = _ffi.BprSampleStats()
            _ffi.check(_ffi.load().fmhip_bpr_resample(self.handle, operator.index(t), C.byref(st)))
        else:
            st = _ffi.BprAdaptiveStats()
            _ffi.check(_ffi.load().fmhip_bpr_resample_adaptive(fm.handle, self.handle, operator.index(t), C.byref(st)))
        self.sample_stats = st.as_dict()
        return self.sample_stats

    def candidate_draws(self, fm, t, p0=0, p1=None):
        """(rows int32, scores float32), each [p1 - p0, n_candidates]: what the adaptive sampler sees for the pairs [p0, p1) at epoch
        `t` under `fm` — every candidate's row and its score yq_i + <q_u, q_i> (fmhip_bpr_debug_adaptive).  Changes no draw."""
        if self.warp:
            raise ValueError("sampler='warp': candidate_draws is the adaptive sampler's record — use warp_draws(fm, t)")
        p0, p1 = self._pair_range(p0, p1)
        rows = np.empty((p1 - p0, self._n_candidates), np.int32)
        scores = np.empty((p1 - p0, self._n_candidates), np.float32)
        _ffi.check(_ffi.load().fmhip_bpr_debug_adaptive(fm.handle, self.handle, operator.index(t), p0, p1, _ffi.ptr(rows), _ffi.ptr(scores)))
        return rows, scores

    def _pair_range(self, p0, p1):
        p0 = operator.index(p0)
        p1 = self.n_pairs if p1 is None else operator.index(p1)
        if not 0 <= p0 < p1 <= self.n_pairs:
            raise ValueError("pairs [%d, %d) must be a non-empty range inside [0, %d)" % (p0, p1, self.n_pairs))
        return p0, p1

    def _need_warp(self, what):
        if not self.warp:
            raise ValueError("%s belongs to sampler='warp', not %r" % (what, self._sampler))

    def warp_draws(self, fm, t, p0=0, p1=None):
        """(rows int32 [p1 - p0, n_candidates], scores float32 of the same shape, pos_scores float32 [p1 - p0]): what the WARP
        sampler sees for the pairs [p0, p1) at epoch `t` under `fm` — every candidate's row and score and the positive's score s+
        (fmhip_warp_debug).  Changes no draw."""
        self._need_warp("warp_draws")
        p0, p1 = self._pair_range(p0, p1)
        rows = np.empty((p1 - p0, self._n_candidates), np.int32)
        scores = np.empty((p1 - p0, self._n_candidates), np.float32)
        pos = np.empty(p1 - p0, np.float32)
        _ffi.check(_ffi.load().fmhip_warp_debug(fm.handle, self.handle, operator.index(t), p0, p1, _ffi.ptr(rows), _ffi.ptr(scores), _ffi.ptr(pos)))
        return rows, scores, pos

    def pair_weights(self):
        """float32 [n_pairs]: the standing WARP draw's pair weights c_p = W[N_p] (0 where no candidate violated)."""
        self._need_warp("pair_weights")
        out = np.empty(self.n_pairs, np.float32)
        _ffi.check(_ffi.load().fmhip_warp_weights(self.handle, _ffi.ptr(out)))
        return out

    def trials(self):
        """int32 [n_pairs]: the standing WARP draw's N_p — 1 + the index of the first violating candidate, 0 for none."""
        self._need_warp("trials")
        out = np.empty(self.n_pairs, np.int32)
        _ffi.check(_ffi.load().fmhip_warp_trials(self.handle, _ffi.ptr(out)))
        return out

    def negatives(self):
        """int32 [n_pairs]: the current draw (the draw at t = 0 until the first resample or learn)."""
        out = np.empty(self.n_pairs, np.int32)
        _ffi.check(_ffi.load().fmhip_bpr_negatives(self.handle, _ffi.ptr(out)))
        return out

    def pairs(self):
        """(ctx, pos, neg) row arrays [n_pairs], in training order."""
        return np.repeat(self.inter_ctx, self.n_neg), np.repeat(self.inter_cand, self.n_neg), self.negatives()

    def expand(self):
        """The flat ``DataSet.from_pairs`` of the current draw: row 2p = context ++ positive (label 1), row 2p+1 = context ++
        negative (label 0), batched by 2 * batch_pairs rows.  For tests and for comparison with the flat route."""
        ctx, pos, neg = self.pairs()
        n = 2 * self.n_pairs
        u = np.repeat(ctx.astype(np.int64), 2)
        i = np.empty(n, np.int64)
        i[0::2], i[1::2] = pos, neg
        srcs = [(self.contexts, u), (self.candidates, i)]
        lens = [blk.row_ptr[mp + 1] - blk.row_ptr[mp] for blk, mp in srcs]
        row_ptr = np.zeros(n + 1, np.int64)
        np.cumsum(lens[0] + lens[1], out=row_ptr[1:])
        col, val = np.empty(row_ptr[-1], np.int32), np.empty(row_ptr[-1], np.float64)
        at = row_ptr[:-1].copy()
        for (blk, mp), ln in zip(srcs, lens):
            within = np.arange(ln.sum(), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
            src, dst = np.repeat(blk.row_ptr[mp], ln) + within, np.repeat(at, ln) + within
            col[dst], val[dst] = blk.col[src], blk.val[src]
            at += ln
        y = np.zeros(n)
        y[0::2] = 1.0
        return DataSet(row_ptr, col, val, y, name="bpr.flat", batch_rows=2 * self.batch_pairs, device=self.device)

    # -- training ---------------------------------------------------------------------------
    def _set_rule(self, fm):
        """The model's loss and optimizer (never its pairing flag: the calls are pairwise by construction)."""
        L = _ffi.load()
        if not self.warp and not self._softmax:      # (WARP and the softmax train their own rule: the model's loss is left as it is)
            _ffi.check(L.fmhip_model_set_loss(fm.handle, self._loss_code))
        _ffi.check(L.fmhip_model_set_optimizer(fm.handle, self._opt_code, self.adagrad_eps, self.adagrad_init))

    def learn(self, fm, dataset=None):
        """One epoch (fmhip_bpr_epoch) at t = the epochs done.  redraw="epoch": resample (adaptively under `fm` when n_candidates > 1),
        then every batch in order.  redraw="batch": per batch in order its draw under `fm` as it stands, then its step;
        ``sample_stats`` then holds the sampler's counters summed over the batches (fmhip_redraw_epoch_stats).  `dataset` is not read."""
        st = _ffi.Stats()
        self._set_rule(fm)
        _ffi.check(_ffi.load().fmhip_bpr_epoch(fm.handle, self.handle, self._epoch, self.eta, self.reg0, self.regw, self.regv, None,
                                               C.byref(st)))
        if self._redraw == "batch":
            dr = _ffi.RedrawStats()
            _ffi.check(_ffi.load().fmhip_redraw_epoch_stats(self.handle, C.byref(dr)))
            self.sample_stats = dr.as_dict()
        fm._device_updated()
        self._epoch += 1
        self.last_stats = st.as_dict()
        return fm

    def step(self, fm, batch, t=None, want_stats=True):
        """A single mini-batch step.  Without `t`: on the current draw (fmhip_bpr_step).  With `t`: the batch's pairs are first
        redrawn at epoch `t` under `fm` as it stands, by the trainer's sampler, and the batch's inverse map rebuilt
        (fmhip_redraw_step; either redraw mode); with want_stats ``sample_stats`` holds that draw's counters."""
        if isinstance(t, bool):
            raise TypeError("t must be an epoch index, not %r (want_stats is a keyword)" % (t,))
        st = _ffi.Stats()
        self._set_rule(fm)
        if t is None:
            _ffi.check(_ffi.load().fmhip_bpr_step(fm.handle, self.handle, operator.index(batch), self.eta, self.reg0, self.regw, self.regv,
                                                  C.byref(st) if want_stats else None))
        else:
            dr = _ffi.RedrawStats()
            _ffi.check(_ffi.load().fmhip_redraw_step(fm.handle, self.handle, operator.index(t), operator.index(batch), self.eta, self.reg0,
                                                     self.regw, self.regv, C.byref(st) if want_stats else None,
                                                     C.byref(dr) if want_stats else None))
            if want_stats:
                self.sample_stats = dr.as_dict()
        fm._device_updated()
        if want_stats:
            self.last_stats = st.as_dict()
        return st.as_dict() if want_stats else None

    def fit(self, k, epochs, seed=0, init=None):
        """A model of the trainer's `dimension` with `k` factors, trained for `epochs` epochs.  `init` = (w0, w, v)."""
        fm = FMModel(self.dimension, k, seed=seed, device=self.device)
        if init is not None:
            fm.w0, fm.w, fm.v = init
        for _ in range(operator.index(epochs)):
            fm = self.learn(fm)
        return fm

    # -- scores of the current pairs -------------------------------------------------------------
    def _pair_score(self, fm):
        ll, conc = C.c_double(), C.c_double()
        _ffi.check(_ffi.load().fmhip_bpr_pair_logloss(fm.handle, self.handle, C.byref(ll), C.byref(conc), None))
        return ll.value, conc.value

    @property
    def softmax(self):
        """True with loss="softmax"."""
        return self._softmax

    @property
    def logq(self):
        """None unless the log-Q correction is in force (loss="softmax", logq=True, a weighted proposal), else the float32 [M]
        table log(w_i / sum w) the logits are corrected by (fmhip_softmax_logq)."""
        if not (self._softmax and self._logq and self._proposal is not None):
            return None
        out = np.empty(self.candidates.size, np.float32)
        _ffi.check(_ffi.load().fmhip_softmax_logq(self.handle, _ffi.ptr(out)))
        return out

    def softmax_probs(self):
        """float32 [n_pairs]: the softmax probability of every pair's negative as the last step of its batch left it
        (fmhip_softmax_probs); every batch must have had a step."""
        if not self._softmax:
            raise ValueError("softmax_probs belongs to loss='softmax', not %r" % (self.loss,))
        out = np.empty(self.n_pairs, np.float32)
        _ffi.check(_ffi.load().fmhip_softmax_probs(self.handle, _ffi.ptr(out)))
        return out

    def _softmax_score(self, fm):
        loss, top1 = C.c_double(), C.c_double()
        _ffi.check(_ffi.load().fmhip_softmax_loss(fm.handle, self.handle, C.byref(loss), C.byref(top1), None))
        return loss.value, top1.value

    def computeSoftmaxLoss(self, fm):
        """Mean over the interactions of -log softmax(s+ | s+, the interaction's n_neg current negatives) (fmhip_softmax_loss),
        log-Q corrected when the correction is in force."""
        return self._softmax_score(fm)[0]

    def computeTop1(self, fm):
        """Share of the interactions whose positive scores strictly above all of its n_neg current negatives."""
        return self._softmax_score(fm)[1]

    def computePairLogLoss(self, fm):
        """Mean -log sigmoid(yhat(u, i+) - yhat(u, i-)) over the current pairs (fmhip_bpr_pair_logloss)."""
        return self._pair_score(fm)[0]

    def computePairAccuracy(self, fm):
        """Share of the current pairs whose positive the model scores higher (a tie counts one half)."""
        return self._pair_score(fm)[1]
