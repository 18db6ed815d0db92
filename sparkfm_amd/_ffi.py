"""ctypes binding of libfmhip.so — the same C ABI (include/fmhip.h, include/fmhip_experimental.h, include/fmhip_topk.h, include/fmhip_pairing.h, include/fmhip_metrics.h, include/fmhip_ranking.h, include/fmhip_weights.h, include/fmhip_relational.h, include/fmhip_mcmc.h, include/fmhip_mcmc_task.h, include/fmhip_mcmc_groups.h, include/fmhip_mcmc_relational.h, include/fmhip_bpr.h, include/fmhip_bpr_adaptive.h, include/fmhip_warp.h, include/fmhip_ftrl.h, include/fmhip_redraw.h, include/fmhip_sgda.h) a JNI shim would bind.

There is NO CPU fallback: if the HIP library is missing this module raises, loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMHIP_LIB") or os.path.join(_HERE, "lib", "libfmhip.so")   # FMHIP_LIB: A/B builds

OK = 0
K_FORWARD, K_REDUCE, K_BACKWARD, K_FIXUP, K_APPLY, K_COUNT = 0, 1, 2, 3, 4, 5
KERNEL_NAMES = ("forward", "reduce", "backward", "fixup", "apply")
RANGE_LEN = 64

# every symbol include/fmhip.h declares — the PRODUCT surface (tests check the library exports all of them)
SYMBOLS = (
    "fmhip_version", "fmhip_last_error", "fmhip_device_count",
    "fmhip_model_create", "fmhip_model_destroy", "fmhip_model_info", "fmhip_model_init_normal",
    "fmhip_model_set_params", "fmhip_model_get_params", "fmhip_model_get_rows", "fmhip_model_set_params_f32", "fmhip_model_get_params_f32",
    "fmhip_synchronize", "fmhip_model_set_loss", "fmhip_model_set_optimizer",
    "fmhip_dataset_create", "fmhip_dataset_create_f32", "fmhip_dataset_create_opts", "fmhip_rows_create", "fmhip_rows_create_f32",
    "fmhip_dataset_destroy", "fmhip_dataset_info", "fmhip_dataset_batch_info", "fmhip_dataset_get_transpose",
    "fmhip_predict", "fmhip_predict_rows", "fmhip_rmse", "fmhip_logloss", "fmhip_residual", "fmhip_term_q",
    "fmhip_sgd_step", "fmhip_sgd_epoch", "fmhip_batch_grad", "fmhip_als_epoch",
    "fmhip_grad_floats", "fmhip_grad_bind", "fmhip_grad_ptr", "fmhip_grad_layout", "fmhip_step_compute",
    "fmhip_step_forward", "fmhip_step_backward", "fmhip_step_apply", "fmhip_step_stats",
    "fmhip_comm_unique_id", "fmhip_comm_create", "fmhip_comm_destroy", "fmhip_comm_info", "fmhip_comm_selftest",
    "fmhip_dp_exchange", "fmhip_dp_exchange_info", "fmhip_dp_plan", "fmhip_dp_plan_info",
    "fmhip_dp_step", "fmhip_dp_step_at", "fmhip_dp_steps", "fmhip_dp_epoch", "fmhip_dp_epoch_order", "fmhip_shard_rows",
    "fmhip_feature_counts", "fmhip_rank_from_counts", "fmhip_relabel_columns",
    "fmhip_feature_counts_gpu", "fmhip_rank_from_counts_gpu", "fmhip_relabel_columns_gpu",
)
# ... and include/fmhip_experimental.h — the measurement / experiment surface (tuning keys, profiling, emulation, layout
# queries, the two-pass forward on its own, a transport of the caller's own)
SYMBOLS_EXPERIMENTAL = (
    "fmhip_ablation_mask", "fmhip_tune", "fmhip_model_tune",
    "fmhip_profile_begin", "fmhip_profile_begin_rotating", "fmhip_profile_begin_sampled", "fmhip_profile_end",
    "fmhip_dataset_layout", "fmhip_dataset_hot_pages", "fmhip_dataset_band_plan", "fmhip_dataset_als_levels",
    "fmhip_dataset_partition_rows", "fmhip_step_forward_pass",
    "fmhip_comm_create_external", "fmhip_stream_wait", "fmhip_device_read", "fmhip_device_write",
    "fmhip_comm_profile_begin", "fmhip_comm_profile_end", "fmhip_comm_emulate", "fmhip_comm_emulate_load", "fmhip_comm_emulate_ranks",
    "fmhip_model_get_optimizer_state", "fmhip_model_set_optimizer_state", "fmhip_bpr_debug_inverse", "fmhip_bpr_debug_adaptive",
    "fmhip_warp_debug",
)
# ... and include/fmhip_topk.h — top-K recommendation over (contexts x candidates)
SYMBOLS_TOPK = ("fmhip_topk", "fmhip_pair_scores")
TOPK_MAX = 128      # FMHIP_TOPK_MAX
# ... and include/fmhip_pairing.h — pairwise ranking: training on pairs of adjacent rows, scoring held-out pairs
SYMBOLS_PAIRING = ("fmhip_model_set_pairing", "fmhip_pair_logloss")
# ... and include/fmhip_metrics.h — ranking metrics: ROC AUC and per-group AUC, exact
SYMBOLS_METRICS = ("fmhip_auc_scores", "fmhip_auc")
# ... and include/fmhip_ranking.h — ranking evaluation: exact ranks of given candidate rows, HR / NDCG / MRR / MAP from them
SYMBOLS_RANKING = ("fmhip_rank", "fmhip_rank_metrics")
# ... and include/fmhip_weights.h — per-row example weights: weighted datasets, weighted scores
SYMBOLS_WEIGHTS = ("fmhip_dataset_create_weighted", "fmhip_rows_create_weighted", "fmhip_dataset_weights", "fmhip_weighted_scores")
# ... and include/fmhip_relational.h — relational data: block-structure FM training and scoring
SYMBOLS_RELATIONAL = ("fmhip_relational_create", "fmhip_relational_destroy", "fmhip_relational_info", "fmhip_relational_predict",
                      "fmhip_relational_rmse", "fmhip_relational_logloss", "fmhip_relational_sgd_step", "fmhip_relational_sgd_epoch")
RELATIONS_MAX = 8          # FMHIP_RELATIONS_MAX
RELATIONAL_SUM_CUT = 256   # FMHIP_RELATIONAL_SUM_CUT: a block row referenced by more rows of a batch is summed in chunks of this many
# ... and include/fmhip_mcmc.h — the MCMC learner: Bayesian FM by Gibbs sampling on the ALS column walk
SYMBOLS_MCMC = ("fmhip_mcmc_opts_default", "fmhip_mcmc_create", "fmhip_mcmc_destroy", "fmhip_mcmc_epoch", "fmhip_mcmc_get_state",
                "fmhip_mcmc_set_state", "fmhip_mcmc_reset_average", "fmhip_mcmc_predictions")
# ... and include/fmhip_mcmc_task.h — its tasks: probit classification with truncated-normal targets, the regression clamp
SYMBOLS_MCMC_TASK = ("fmhip_mcmc_task_opts_default", "fmhip_mcmc_create_task", "fmhip_mcmc_latent_targets")
MCMC_REGRESSION, MCMC_CLASSIFICATION = 0, 1
# ... and include/fmhip_mcmc_groups.h — its attribute groups: a lambda and a mu per feature group
SYMBOLS_MCMC_GROUPS = ("fmhip_mcmc_set_groups", "fmhip_mcmc_group_info", "fmhip_mcmc_get_group_state", "fmhip_mcmc_set_group_state")
MCMC_MAX_GROUPS = 4096     # FMHIP_MCMC_MAX_GROUPS
# ... and include/fmhip_mcmc_relational.h — its block-structure sweep over relational data
SYMBOLS_MCMC_RELATIONAL = ("fmhip_mcmc_create_relational",)
# ... and include/fmhip_bpr.h — the BPR trainer: negatives drawn on the device over a contexts and a candidates block
SYMBOLS_BPR = ("fmhip_bpr_create", "fmhip_bpr_destroy", "fmhip_bpr_info", "fmhip_bpr_resample", "fmhip_bpr_negatives", "fmhip_bpr_step",
               "fmhip_bpr_epoch", "fmhip_bpr_pair_logloss")
# ... and include/fmhip_bpr_adaptive.h — its adaptive negatives: C candidates per pair, the model's best kept
SYMBOLS_BPR_ADAPTIVE = ("fmhip_bpr_set_candidates", "fmhip_bpr_get_candidates", "fmhip_bpr_resample_adaptive")
BPR_MAX_CANDIDATES = 64    # FMHIP_BPR_MAX_CANDIDATES
# ... and include/fmhip_warp.h — WARP: the first candidate that violates the margin, a hinge weighted by the estimated rank
SYMBOLS_WARP = ("fmhip_warp_set", "fmhip_warp_get", "fmhip_warp_resample", "fmhip_warp_weights", "fmhip_warp_trials")
# ... and include/fmhip_redraw.h — when the BPR trainer redraws: once per epoch, or before every batch under the current model
SYMBOLS_REDRAW = ("fmhip_redraw_set", "fmhip_redraw_get", "fmhip_redraw_step", "fmhip_redraw_epoch_stats")
REDRAW_EPOCH, REDRAW_BATCH = 0, 1      # FMHIP_REDRAW_EPOCH, FMHIP_REDRAW_BATCH
REDRAWS = {"epoch": REDRAW_EPOCH, "batch": REDRAW_BATCH}
# ... and include/fmhip_ftrl.h — FTRL-Proximal with L1: the third update rule, its state, the model's exact sparsity counts
SYMBOLS_FTRL = ("fmhip_model_set_ftrl", "fmhip_model_get_ftrl_state", "fmhip_model_set_ftrl_state", "fmhip_model_nonzeros")
# ... and include/fmhip_sgda.h — SGDA: SGD whose per-group regularisers take gradient steps on a validation set
SYMBOLS_SGDA = ("fmhip_sgda_create", "fmhip_sgda_destroy", "fmhip_sgda_step", "fmhip_sgda_epoch", "fmhip_sgda_get_lambda",
                "fmhip_sgda_set_lambda", "fmhip_sgda_last_sums", "fmhip_sgda_info")
SGDA_MAX_GROUPS = 4096     # FMHIP_SGDA_MAX_GROUPS
# ... and include/fmhip_proposal.h — what the BPR trainer draws candidate rows from: uniform, or an alias table of M weights
SYMBOLS_PROPOSAL = ("fmhip_proposal_set", "fmhip_proposal_get", "fmhip_proposal_table")
# ... and include/fmhip_softmax.h — the sampled softmax over an interaction's n_neg negatives, with the proposal's log-Q correction
SYMBOLS_SOFTMAX = ("fmhip_softmax_set", "fmhip_softmax_get", "fmhip_softmax_loss", "fmhip_softmax_probs", "fmhip_softmax_logq")
OPT_FTRL = 2               # FMHIP_OPT_FTRL: reported, never accepted by fmhip_model_set_optimizer (not in OPTIMIZERS)
# enum fmhip_tune_key (include/fmhip_experimental.h); TUNE maps the names without their prefix
(TUNE_FORWARD_KERNEL, TUNE_BACKWARD_KERNEL, TUNE_TILE_ROWS, TUNE_ROW_BLOCK, TUNE_XCD_PLACEMENT, TUNE_HOT_BLOCK, TUNE_FORWARD_OCCUPANCY,
 TUNE_ROW_ORDER, TUNE_FLAT_ADDRESS, TUNE_LAZY_DECAY, TUNE_FUSED_UPDATE, TUNE_MERGED_FINISH, TUNE_HOT_PAGES) = range(13)
TUNE = {name[5:]: value for name, value in list(globals().items()) if name.startswith("TUNE_")}
# values of FORWARD_KERNEL: the kernel, plus FWD_NO_ISSUE_PRIO for the w-tile kernel's instance without the raised issue priority
FWD_WTILE, FWD_VTILE, FWD_PLAIN, FWD_NO_ISSUE_PRIO, FWD_DEFAULT = 60, 20, 0, 1, 60
UNIQUE_ID_BYTES = 128
# enum fmhip_loss (include/fmhip.h): the loss a model trains under (fmhip_model_set_loss)
LOSS_SQUARED, LOSS_LOGISTIC = 0, 1
LOSSES = {"squared": LOSS_SQUARED, "logistic": LOSS_LOGISTIC}


def loss_code(loss):
    """'squared' | 'logistic' -> enum fmhip_loss; anything else raises ValueError."""
    if loss not in LOSSES:
        raise ValueError("loss must be one of %s, not %r" % (sorted(LOSSES), loss))
    return LOSSES[loss]


# enum fmhip_pairing (include/fmhip_pairing.h): how a batch's rows form the examples a model trains on (fmhip_model_set_pairing)
PAIRING_NONE, PAIRING_ADJACENT = 0, 1


def pairing_code(pairs):
    """False | True -> enum fmhip_pairing; anything but a bool raises ValueError."""
    if not isinstance(pairs, bool):
        raise ValueError("pairs must be True or False, not %r" % (pairs,))
    return PAIRING_ADJACENT if pairs else PAIRING_NONE


# enum fmhip_optimizer (include/fmhip.h): the update rule a model trains under (fmhip_model_set_optimizer)
OPT_SGD, OPT_ADAGRAD = 0, 1
OPTIMIZERS = {"sgd": OPT_SGD, "adagrad": OPT_ADAGRAD}


def optimizer_code(optimizer):
    """'sgd' | 'adagrad' -> enum fmhip_optimizer; anything else raises ValueError."""
    if optimizer not in OPTIMIZERS:
        raise ValueError("optimizer must be one of %s, not %r" % (sorted(OPTIMIZERS), optimizer))
    return OPTIMIZERS[optimizer]


def adagrad_settings(eps, init):
    """(eps, initial accumulator) as floats; ValueError unless eps is finite and > 0 and init finite and >= 0 (as the C ABI)."""
    import math
    eps, init = float(eps), float(init)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("adagrad_eps must be finite and > 0, not %r" % eps)
    if not (math.isfinite(init) and init >= 0.0):
        raise ValueError("adagrad_init must be finite and >= 0, not %r" % init)
    return eps, init


class TrainRule:
    """How a model trains, as one value: loss, optimizer with its AdaGrad settings, pairing — the learners' five keywords,
    validated here (ValueError); `set_on` puts it on a model through the three setters of the C ABI."""

    def __init__(self, loss="squared", optimizer="sgd", adagrad_eps=1e-10, adagrad_init=0.1, pairs=False):
        self.loss, self.optimizer, self.pairs = loss, optimizer, pairs
        self.loss_code, self.opt_code = loss_code(loss), optimizer_code(optimizer)
        self.adagrad_eps, self.adagrad_init = adagrad_settings(adagrad_eps, adagrad_init)
        self.pairing_code = pairing_code(pairs)

    def publish(self, learner):
        """The keywords as the learner's public attributes (.loss, .optimizer, .adagrad_eps, .adagrad_init, .pairs) -> self."""
        for name in ("loss", "optimizer", "adagrad_eps", "adagrad_init", "pairs"):
            setattr(learner, name, getattr(self, name))
        return self

    def set_on(self, handle):
        """fmhip_model_set_loss, _set_pairing, _set_optimizer (the same AdaGrad settings again keep the model's accumulators)."""
        L = load()
        check(L.fmhip_model_set_loss(handle, self.loss_code))
        check(L.fmhip_model_set_pairing(handle, self.pairing_code))
        check(L.fmhip_model_set_optimizer(handle, self.opt_code, self.adagrad_eps, self.adagrad_init))

    def require_default(self):
        """For a step engine that cannot set a rule: ValueError for every part that is not the default."""
        if self.loss_code != LOSS_SQUARED:
            raise ValueError("this engine trains the squared loss only")
        if self.pairing_code != PAIRING_NONE:
            raise ValueError("this engine trains on single rows only")
        if self.opt_code != OPT_SGD:
            raise ValueError("this engine trains with plain SGD only")


def ftrl_settings(beta, init, l1w, l1v):
    """(beta, initial accumulator, l1w, l1v) as floats; ValueError unless all are finite and >= 0 and beta + sqrt(init) > 0 (as the
    C ABI, which checks the sum in fp32)."""
    import math
    import struct
    out = []
    for name, x in (("beta", beta), ("ftrl_init", init), ("l1w", l1w), ("l1v", l1v)):
        x = float(x)
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, x))
        out.append(x)
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    if not f32(out[0]) + math.sqrt(f32(out[1])) > 0.0:
        raise ValueError("beta + sqrt(ftrl_init) must be > 0 (the first step would divide by zero), not beta %r, ftrl_init %r" % (out[0], out[1]))
    return tuple(out)


class FtrlRule(TrainRule):
    """A TrainRule whose update rule is FTRL-Proximal (include/fmhip_ftrl.h): loss and pairing as TrainRule's, the rule's four
    settings validated here (ValueError); `set_on` puts it on a model through fmhip_model_set_ftrl (the same settings again keep
    the model's zeta and n)."""

    def __init__(self, loss="squared", pairs=False, beta=1.0, ftrl_init=0.0, l1w=0.0, l1v=0.0):
        super().__init__(loss=loss, pairs=pairs)
        self.optimizer, self.opt_code = "ftrl", OPT_FTRL
        self.beta, self.ftrl_init, self.l1w, self.l1v = ftrl_settings(beta, ftrl_init, l1w, l1v)

    def publish(self, learner):
        """The keywords as the learner's public attributes (.loss, .pairs, .beta, .ftrl_init, .l1w, .l1v) -> self."""
        for name in ("loss", "pairs", "beta", "ftrl_init", "l1w", "l1v"):
            setattr(learner, name, getattr(self, name))
        return self

    def set_on(self, handle):
        """fmhip_model_set_loss, _set_pairing, _set_ftrl."""
        L = load()
        check(L.fmhip_model_set_loss(handle, self.loss_code))
        check(L.fmhip_model_set_pairing(handle, self.pairing_code))
        check(L.fmhip_model_set_ftrl(handle, self.beta, self.ftrl_init, self.l1w, self.l1v))


class Stats(C.Structure):
    _fields_ = [("sse", C.c_double), ("sum_e", C.c_double), ("rows", C.c_int64), ("nnz", C.c_int64),
                ("nonfinite", C.c_int64), ("steps", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * K_COUNT), ("launches", C.c_int64 * K_COUNT), ("nnz", C.c_int64 * K_COUNT),
                ("rows", C.c_int64 * K_COUNT), ("steps", C.c_int64 * K_COUNT)]

    def as_dict(self):
        return {KERNEL_NAMES[i]: dict(ms=self.ms[i], launches=self.launches[i], nnz=self.nnz[i], rows=self.rows[i], steps=self.steps[i])
                for i in range(K_COUNT)}


class AucResult(C.Structure):
    """fmhip_auc_result (include/fmhip_metrics.h); struct_size is filled in on construction."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("u2", C.c_uint64), ("pairs", C.c_int64),
                ("positives", C.c_int64), ("negatives", C.c_int64), ("groups", C.c_int64), ("groups_scored", C.c_int64),
                ("auc", C.c_double), ("gauc", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(AucResult)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}


class RankMetrics(C.Structure):
    """fmhip_rank_metrics_t (include/fmhip_ranking.h); struct_size is filled in on construction."""
    _fields_ = [("struct_size", C.c_int32), ("k", C.c_int32), ("contexts", C.c_int64), ("skipped", C.c_int64), ("relevant", C.c_int64),
                ("hit_rate", C.c_double), ("recall", C.c_double), ("precision", C.c_double), ("ndcg", C.c_double),
                ("mrr", C.c_double), ("map", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(RankMetrics)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class WeightedResult(C.Structure):
    """fmhip_weighted_result (include/fmhip_weights.h); struct_size is filled in on construction."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("sum_w", C.c_double), ("rmse", C.c_double), ("mae", C.c_double),
                ("logloss", C.c_double), ("rows", C.c_int64), ("nonfinite", C.c_int64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(WeightedResult)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}


def row_weights(weights, n):
    """None | n numbers -> None | a contiguous float64 array (ValueError: wrong length).  Their values — finite, >= 0 — are the
    library's to check: it names the first offending row."""
    if weights is None:
        return None
    import numpy as np
    w = np.ascontiguousarray(weights, np.float64)
    if w.shape != (n,):
        raise ValueError("weights must hold one weight per row (%d), not shape %r" % (n, w.shape))
    return w


def row_lists(lists, n_contexts, n_candidates, what):
    """One integer array of candidate rows per context -> (ptr int64 [n_contexts + 1], rows int32): the lists sorted and
    de-duplicated, one after the other; ValueError for a wrong count or a row outside [0, n_candidates).  `rows` is never empty
    (a non-NULL pointer): its ptr[n_contexts] leading entries count.  All lists are handled in one pass (thousands of short
    lists cost more in per-list numpy calls than the device takes to rank them)."""
    import numpy as np
    if len(lists) != n_contexts:
        raise ValueError("%s must hold one array per context (%d), not %d" % (what, n_contexts, len(lists)))
    lists = [np.asarray(e).reshape(-1) for e in lists]
    lens = np.fromiter((len(e) for e in lists), np.int64, n_contexts)
    ptr = np.zeros(n_contexts + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate(lists).astype(np.int64, copy=False) if ptr[-1] else np.zeros(0, np.int64)
    if len(flat) and (flat.min() < 0 or flat.max() >= n_candidates):
        raise ValueError("%s names a candidate row outside [0, %d)" % (what, n_candidates))
    # lists that come ascending and distinct (every step inside a list goes up) are taken as they stand
    up = flat[1:] > flat[:-1]
    heads = ptr[1:-1]
    up[heads[(heads > 0) & (heads < len(flat))] - 1] = True
    if not up.all():
        key = np.unique(np.repeat(np.arange(n_contexts, dtype=np.int64), lens) * int(n_candidates) + flat)      # (context, row)
        np.cumsum(np.bincount(key // int(n_candidates), minlength=n_contexts), out=ptr[1:])
        flat = key % int(n_candidates)
    rows = np.ascontiguousarray(flat, np.int32)
    if not len(rows):
        rows = np.zeros(1, np.int32)
    return ptr, rows


def group_ids(groups, n):
    """None | n integers -> None | a contiguous int32 array (ValueError: wrong length, an id outside [0, 2^31))."""
    if groups is None:
        return None
    import numpy as np
    g = np.asarray(groups)
    if g.shape != (n,):
        raise ValueError("groups must hold one id per row (%d), not shape %r" % (n, g.shape))
    if n and not np.issubdtype(g.dtype, np.integer):
        raise ValueError("groups must be integers, not %s" % g.dtype)
    if n and int(g.max()) >= 2 ** 31:
        raise ValueError("group ids must be below 2^31")
    if n and int(g.min()) < -2 ** 31:
        raise ValueError("group ids must be >= 0")
    return np.ascontiguousarray(g, np.int32)     # (a negative id is refused by the library, which names the row)


class McmcOpts(C.Structure):
    """fmhip_mcmc_opts (include/fmhip_mcmc.h)."""
    _fields_ = [("seed", C.c_uint64), ("sample", C.c_int32), ("reg0", C.c_double), ("init_lambda", C.c_double),
                ("alpha_0", C.c_double), ("beta_0", C.c_double), ("alpha_lambda", C.c_double), ("beta_lambda", C.c_double),
                ("gamma_0", C.c_double), ("mu_0", C.c_double)]


class McmcTaskOpts(C.Structure):
    """fmhip_mcmc_task_opts (include/fmhip_mcmc_task.h)."""
    _fields_ = [("task", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_double), ("clip_hi", C.c_double)]


class McmcStats(C.Structure):
    """fmhip_mcmc_stats (include/fmhip_mcmc.h)."""
    _fields_ = [("alpha", C.c_double), ("train_rmse", C.c_double), ("iterations", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BprSampleStats(C.Structure):
    """fmhip_bpr_sample_stats (include/fmhip_bpr.h)."""
    _fields_ = [("attempts", C.c_int64), ("forced", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BprAdaptiveStats(C.Structure):
    """fmhip_bpr_adaptive_stats (include/fmhip_bpr_adaptive.h)."""
    _fields_ = [("attempts", C.c_int64), ("forced", C.c_int64), ("replaced", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WarpStats(C.Structure):
    """fmhip_warp_stats (include/fmhip_warp.h)."""
    _fields_ = [("pairs", C.c_int64), ("violated", C.c_int64), ("trials", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RedrawStats(C.Structure):
    """fmhip_redraw_stats (include/fmhip_redraw.h)."""
    _fields_ = [("pairs", C.c_int64), ("attempts", C.c_int64), ("forced", C.c_int64), ("replaced", C.c_int64), ("violated", C.c_int64),
                ("trials", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DatasetOpts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hot_block", C.c_int32), ("batch_rows", C.c_int64), ("row_block_rows", C.c_int64)]


# int fn(void *ctx, void *device_buf, size_t count, int kind, void *hip_stream) — fmhip_comm_create_external
CollectiveFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
COLL_SUM_F32, COLL_MAX_I64, COLL_BCAST0_I64, COLL_ALLGATHER_I32, COLL_REDUCE_SCATTER_F32, COLL_ALLGATHER_F32 = 0, 1, 2, 3, 4, 5
EXCHANGE_DENSE, EXCHANGE_TOUCHED, EXCHANGE_SHARDED = 0, 1, 2
EXCHANGE_PIPELINED = 3
EXCHANGE_MODES = {"dense": EXCHANGE_DENSE, "touched": EXCHANGE_TOUCHED, "sharded": EXCHANGE_SHARDED, "pipelined": EXCHANGE_PIPELINED}


class CommProfile(C.Structure):
    _fields_ = [("exposed_ms", C.c_double), ("comm_ms", C.c_double), ("steps", C.c_int64), ("bytes", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FmhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fmhip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Loads libfmhip.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libfmhip.so not found at %s — build it first: python -c 'import __graft_entry__ as g; g.build()' "
            "(sparkfm_amd has no CPU fallback)" % LIB_PATH)
    try:
        # torch bundles its own HIP runtime (same soname); import it first so that one process
        # never ends up with two runtimes when torch tensors/streams are shared with the library
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    P = C.POINTER
    L.fmhip_version.restype = C.c_int
    L.fmhip_last_error.restype = C.c_char_p
    L.fmhip_device_count.argtypes = [P(C.c_int)]
    L.fmhip_tune.argtypes = [C.c_int, C.c_int]
    L.fmhip_model_create.argtypes = [C.c_int, i64, i32, vp, P(vp)]
    L.fmhip_model_destroy.argtypes = [vp]
    L.fmhip_model_tune.argtypes = [vp, C.c_int, C.c_int]
    L.fmhip_model_info.argtypes = [vp, P(i64), P(i32), P(i32)]
    L.fmhip_model_set_params.argtypes = [vp, dbl, vp, vp]
    L.fmhip_model_get_params.argtypes = [vp, P(dbl), vp, vp]
    L.fmhip_model_set_params_f32.argtypes = [vp, C.c_float, vp, vp]
    L.fmhip_model_get_params_f32.argtypes = [vp, P(C.c_float), vp, vp]
    L.fmhip_synchronize.argtypes = [vp]
    L.fmhip_dataset_create.argtypes = [C.c_int, i64, vp, vp, vp, vp, i64, P(vp)]
    L.fmhip_dataset_create_f32.argtypes = [C.c_int, i64, vp, vp, vp, vp, i64, P(vp)]
    L.fmhip_dataset_destroy.argtypes = [vp]
    L.fmhip_dataset_info.argtypes = [vp, P(i64), P(i64), P(i64), P(i64), P(i64)]
    L.fmhip_dataset_batch_info.argtypes = [vp, i64, P(i64), P(i64), P(i64), P(i64)]
    L.fmhip_dataset_get_transpose.argtypes = [vp, i64, vp, vp, vp, vp]
    L.fmhip_predict.argtypes = [vp, vp, vp]
    L.fmhip_rmse.argtypes = [vp, vp, P(dbl), P(Stats)]
    L.fmhip_logloss.argtypes = [vp, vp, P(dbl), P(Stats)]
    L.fmhip_model_set_loss.argtypes = [vp, C.c_int]
    L.fmhip_model_set_pairing.argtypes = [vp, C.c_int]
    L.fmhip_pair_logloss.argtypes = [vp, vp, P(dbl), P(dbl), P(Stats)]
    L.fmhip_model_set_optimizer.argtypes = [vp, C.c_int, dbl, dbl]
    L.fmhip_model_get_optimizer_state.argtypes = [vp, P(dbl), vp, vp]
    L.fmhip_model_set_optimizer_state.argtypes = [vp, dbl, vp, vp]
    L.fmhip_residual.argtypes = [vp, vp, vp]
    L.fmhip_term_q.argtypes = [vp, vp, vp]
    L.fmhip_sgd_step.argtypes = [vp, vp, i64, dbl, dbl, dbl, dbl, P(Stats)]
    L.fmhip_sgd_epoch.argtypes = [vp, vp, dbl, dbl, dbl, dbl, vp, P(Stats)]
    L.fmhip_batch_grad.argtypes = [vp, vp, i64, vp, vp, P(dbl), P(Stats)]
    L.fmhip_als_epoch.argtypes = [vp, vp, dbl, dbl, dbl]
    L.fmhip_grad_floats.argtypes = [vp, P(i64)]
    L.fmhip_grad_bind.argtypes = [vp, vp]
    L.fmhip_grad_ptr.argtypes = [vp, P(vp)]
    L.fmhip_step_compute.argtypes = [vp, vp, i64]
    L.fmhip_step_forward.argtypes = [vp, vp, i64]
    L.fmhip_step_backward.argtypes = [vp, vp, i64, i64, i64, C.c_int]
    L.fmhip_grad_layout.argtypes = [vp, P(i64), P(i64)]
    L.fmhip_step_apply.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.fmhip_step_stats.argtypes = [vp, P(Stats)]
    L.fmhip_profile_begin.argtypes = [vp]
    L.fmhip_profile_begin_rotating.argtypes = [vp]
    L.fmhip_profile_begin_sampled.argtypes = [vp, C.c_int]
    L.fmhip_profile_end.argtypes = [vp, P(Profile)]
    L.fmhip_dataset_create_opts.argtypes = [C.c_int, i64, vp, vp, vp, vp, P(DatasetOpts), P(vp)]
    L.fmhip_dataset_layout.argtypes = [vp, P(i32), vp, P(i64)]
    L.fmhip_model_get_rows.argtypes = [vp, i64, vp, vp, vp]
    L.fmhip_model_init_normal.argtypes = [vp, C.c_uint64, dbl, dbl]
    L.fmhip_rows_create.argtypes = [C.c_int, i64, vp, vp, vp, vp, P(vp)]
    L.fmhip_rows_create_f32.argtypes = [C.c_int, i64, vp, vp, vp, vp, P(vp)]
    L.fmhip_predict_rows.argtypes = [vp, i64, vp, vp, vp, vp]
    L.fmhip_comm_unique_id.argtypes = [vp]
    L.fmhip_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, P(vp)]
    L.fmhip_comm_destroy.argtypes = [vp]
    L.fmhip_comm_info.argtypes = [vp, P(C.c_int), P(C.c_int)]
    L.fmhip_comm_selftest.argtypes = [vp, P(C.c_int)]
    L.fmhip_dataset_partition_rows.argtypes = [vp, i64]
    L.fmhip_step_forward_pass.argtypes = [vp, vp, i64, C.c_int]
    L.fmhip_dp_steps.argtypes = [vp, vp, vp, i64, vp, dbl, dbl, dbl, dbl]
    L.fmhip_dp_plan.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.fmhip_dp_step.argtypes = [vp, vp, i64, vp, dbl, dbl, dbl, dbl]
    L.fmhip_dp_epoch.argtypes = [vp, vp, vp, dbl, dbl, dbl, dbl, P(Stats)]
    L.fmhip_dp_step_at.argtypes = [vp, vp, i64, vp, dbl, dbl, dbl, dbl]
    L.fmhip_dp_epoch_order.argtypes = [vp, vp, vp, dbl, dbl, dbl, dbl, vp, i64, P(Stats)]
    L.fmhip_dp_plan_info.argtypes = [vp, P(i64), P(i64)]
    L.fmhip_dataset_als_levels.argtypes = [vp, P(i64), P(i64), P(i64)]
    L.fmhip_comm_emulate.argtypes = [vp, dbl]
    L.fmhip_comm_emulate_ranks.argtypes = [vp, C.c_int]
    L.fmhip_comm_emulate_load.argtypes = [vp, C.c_int]
    L.fmhip_comm_profile_begin.argtypes = [vp]
    L.fmhip_comm_profile_end.argtypes = [vp, P(CommProfile)]
    L.fmhip_shard_rows.argtypes = [i64, vp, C.c_int, C.c_int, P(i64), P(i64)]
    L.fmhip_comm_create_external.argtypes = [vp, C.c_int, C.c_int, CollectiveFn, vp, P(vp)]
    L.fmhip_dp_exchange.argtypes = [vp, C.c_int]
    L.fmhip_dp_exchange_info.argtypes = [vp, P(C.c_int), P(i64), P(C.c_double)]
    L.fmhip_stream_wait.argtypes = [vp]
    L.fmhip_device_read.argtypes = [vp, vp, C.c_size_t, vp]
    L.fmhip_device_write.argtypes = [vp, vp, C.c_size_t, vp]
    L.fmhip_dataset_hot_pages.argtypes = [vp, P(C.c_int32), P(C.c_int32), vp, P(i64)]
    L.fmhip_dataset_band_plan.argtypes = [vp, P(i64), P(i64), P(i64)]
    L.fmhip_feature_counts.argtypes = [i64, vp, i64, vp]
    L.fmhip_rank_from_counts.argtypes = [i64, vp, vp, vp]
    L.fmhip_relabel_columns.argtypes = [i64, vp, i64, vp, vp]
    L.fmhip_feature_counts_gpu.argtypes = [C.c_int, i64, vp, i64, vp]
    L.fmhip_rank_from_counts_gpu.argtypes = [C.c_int, i64, vp, vp, vp]
    L.fmhip_relabel_columns_gpu.argtypes = [C.c_int, i64, vp, i64, vp, vp]
    L.fmhip_topk.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    L.fmhip_pair_scores.argtypes = [vp, vp, vp, i64, i64, vp]
    L.fmhip_auc_scores.argtypes = [C.c_int, i64, vp, vp, vp, P(AucResult)]
    L.fmhip_auc.argtypes = [vp, vp, vp, P(AucResult), P(Stats)]
    L.fmhip_rank.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fmhip_rank_metrics.argtypes = [i64, vp, vp, i32, P(RankMetrics)]
    L.fmhip_dataset_create_weighted.argtypes = [C.c_int, i64, vp, vp, vp, vp, vp, P(DatasetOpts), P(vp)]
    L.fmhip_rows_create_weighted.argtypes = [C.c_int, i64, vp, vp, vp, vp, vp, P(vp)]
    L.fmhip_dataset_weights.argtypes = [vp, P(C.c_int), P(dbl), vp]
    L.fmhip_weighted_scores.argtypes = [vp, vp, P(WeightedResult)]
    L.fmhip_relational_create.argtypes = [C.c_int, i64, vp, i32, vp, vp, vp, i64, P(vp)]
    L.fmhip_relational_destroy.argtypes = [vp]
    L.fmhip_relational_info.argtypes = [vp, P(i64), P(i64), P(i64), P(i64), P(i32)]
    L.fmhip_relational_predict.argtypes = [vp, vp, vp]
    L.fmhip_relational_rmse.argtypes = [vp, vp, P(dbl), P(Stats)]
    L.fmhip_relational_logloss.argtypes = [vp, vp, P(dbl), P(Stats)]
    L.fmhip_relational_sgd_step.argtypes = [vp, vp, i64, dbl, dbl, dbl, dbl, P(Stats)]
    L.fmhip_relational_sgd_epoch.argtypes = [vp, vp, dbl, dbl, dbl, dbl, vp, P(Stats)]
    L.fmhip_mcmc_opts_default.argtypes = [P(McmcOpts)]
    L.fmhip_mcmc_create.argtypes = [vp, vp, vp, P(McmcOpts), P(vp)]
    L.fmhip_mcmc_destroy.argtypes = [vp]
    L.fmhip_mcmc_epoch.argtypes = [vp, P(McmcStats)]
    L.fmhip_mcmc_get_state.argtypes = [vp, P(dbl), vp, vp, P(i64)]
    L.fmhip_mcmc_set_state.argtypes = [vp, dbl, vp, vp]
    L.fmhip_mcmc_reset_average.argtypes = [vp]
    L.fmhip_mcmc_predictions.argtypes = [vp, vp, vp, P(i64)]
    L.fmhip_mcmc_task_opts_default.argtypes = [P(McmcTaskOpts)]
    L.fmhip_mcmc_create_task.argtypes = [vp, vp, vp, P(McmcOpts), P(McmcTaskOpts), P(vp)]
    L.fmhip_mcmc_latent_targets.argtypes = [vp, vp]
    L.fmhip_mcmc_set_groups.argtypes = [vp, vp, i64, C.c_int32]
    L.fmhip_mcmc_group_info.argtypes = [vp, P(C.c_int32), vp]
    L.fmhip_mcmc_get_group_state.argtypes = [vp, P(dbl), vp, vp, P(i64)]
    L.fmhip_mcmc_set_group_state.argtypes = [vp, dbl, vp, vp]
    L.fmhip_mcmc_create_relational.argtypes = [vp, vp, vp, vp, P(McmcOpts), P(McmcTaskOpts), C.c_int32, P(vp)]
    L.fmhip_bpr_create.argtypes = [C.c_int, vp, vp, i64, vp, vp, i32, i64, C.c_uint64, P(vp)]
    L.fmhip_bpr_destroy.argtypes = [vp]
    L.fmhip_bpr_info.argtypes = [vp, P(i64), P(i64), P(i64), P(i64), P(i32)]
    L.fmhip_bpr_resample.argtypes = [vp, i64, P(BprSampleStats)]
    L.fmhip_bpr_negatives.argtypes = [vp, vp]
    L.fmhip_bpr_step.argtypes = [vp, vp, i64, dbl, dbl, dbl, dbl, P(Stats)]
    L.fmhip_bpr_epoch.argtypes = [vp, vp, i64, dbl, dbl, dbl, dbl, vp, P(Stats)]
    L.fmhip_bpr_pair_logloss.argtypes = [vp, vp, P(dbl), P(dbl), P(Stats)]
    L.fmhip_bpr_debug_inverse.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fmhip_bpr_set_candidates.argtypes = [vp, i32]
    L.fmhip_bpr_get_candidates.argtypes = [vp, P(i32)]
    L.fmhip_bpr_resample_adaptive.argtypes = [vp, vp, i64, P(BprAdaptiveStats)]
    L.fmhip_bpr_debug_adaptive.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    L.fmhip_warp_set.argtypes = [vp, C.c_int, dbl]
    L.fmhip_warp_get.argtypes = [vp, P(C.c_int), P(dbl)]
    L.fmhip_warp_resample.argtypes = [vp, vp, i64, P(WarpStats)]
    L.fmhip_warp_weights.argtypes = [vp, vp]
    L.fmhip_warp_trials.argtypes = [vp, vp]
    L.fmhip_warp_debug.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
    L.fmhip_redraw_set.argtypes = [vp, C.c_int]
    L.fmhip_redraw_get.argtypes = [vp, P(C.c_int)]
    L.fmhip_redraw_step.argtypes = [vp, vp, i64, i64, dbl, dbl, dbl, dbl, P(Stats), P(RedrawStats)]
    L.fmhip_redraw_epoch_stats.argtypes = [vp, P(RedrawStats)]
    L.fmhip_model_set_ftrl.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.fmhip_model_get_ftrl_state.argtypes = [vp, P(dbl), vp, vp, P(dbl), vp, vp]
    L.fmhip_model_set_ftrl_state.argtypes = [vp, dbl, vp, vp, dbl, vp, vp]
    L.fmhip_model_nonzeros.argtypes = [vp, P(i64), P(i64), P(i64)]
    L.fmhip_sgda_create.argtypes = [vp, vp, i64, i32, dbl, dbl, P(vp)]
    L.fmhip_sgda_destroy.argtypes = [vp]
    L.fmhip_sgda_step.argtypes = [vp, vp, i64, vp, i64, dbl, dbl, dbl, P(Stats), P(Stats)]
    L.fmhip_sgda_epoch.argtypes = [vp, vp, vp, dbl, dbl, dbl, vp, P(Stats), P(Stats)]
    L.fmhip_sgda_get_lambda.argtypes = [vp, vp, vp]
    L.fmhip_sgda_set_lambda.argtypes = [vp, vp, vp]
    L.fmhip_sgda_last_sums.argtypes = [vp, vp, vp]
    L.fmhip_sgda_info.argtypes = [vp, P(i32), vp, P(i64)]
    L.fmhip_proposal_set.argtypes = [vp, vp]
    L.fmhip_proposal_get.argtypes = [vp, P(C.c_int)]
    L.fmhip_proposal_table.argtypes = [vp, vp, vp]
    L.fmhip_softmax_set.argtypes = [vp, C.c_int, C.c_int]
    L.fmhip_softmax_get.argtypes = [vp, P(C.c_int), P(C.c_int)]
    L.fmhip_softmax_loss.argtypes = [vp, vp, P(dbl), P(dbl), P(Stats)]
    L.fmhip_softmax_probs.argtypes = [vp, vp]
    L.fmhip_softmax_logq.argtypes = [vp, vp]
    for name in (SYMBOLS + SYMBOLS_EXPERIMENTAL + SYMBOLS_TOPK + SYMBOLS_PAIRING + SYMBOLS_METRICS + SYMBOLS_RANKING + SYMBOLS_WEIGHTS
                 + SYMBOLS_RELATIONAL + SYMBOLS_MCMC + SYMBOLS_MCMC_TASK + SYMBOLS_MCMC_GROUPS + SYMBOLS_MCMC_RELATIONAL + SYMBOLS_BPR + SYMBOLS_BPR_ADAPTIVE
                 + SYMBOLS_WARP + SYMBOLS_FTRL + SYMBOLS_REDRAW + SYMBOLS_SGDA + SYMBOLS_PROPOSAL + SYMBOLS_SOFTMAX):
        fn = getattr(L, name)
        if name not in ("fmhip_version", "fmhip_last_error"):
            fn.restype = C.c_int
    # FMHIP_TUNE="key=value,key=value": experiment knobs (fmhip_tune) applied at load time; key = a number or a name of
    # enum fmhip_tune_key without its prefix (flat_address=1)
    for item in filter(None, os.environ.get("FMHIP_TUNE", "").split(",")):
        k, v = item.split("=")
        L.fmhip_tune(int(k) if k.strip().isdigit() else TUNE[k.strip().upper()], int(v))
    if L.fmhip_ablation_mask() != 0 and not os.environ.get("FMHIP_LIB"):
        raise ImportError("libfmhip.so was built with a timing-only kernel ablation (mask %d): rebuild it without FMHIP_EXP_* flags" % L.fmhip_ablation_mask())
    _lib = L
    return L


def check(code):
    if code != OK:
        raise FmhipError(code, load().fmhip_last_error().decode("utf-8", "replace"))
    return code


def ptr(a):
    """numpy array (or None) -> void* for the C ABI."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)
