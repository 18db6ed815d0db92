"""Ranking metrics of predictions that are already on the host (include/fmhip_metrics.h) — what a data-parallel caller uses
after gathering its ranks' predictions; a model over a dataset goes through ``FMModel.computeAUC`` instead — and of ranks that
are (include/fmhip_ranking.h: ``FMModel.rankOf`` returns them, ``FMModel.computeRankingMetrics`` does both steps)."""
import ctypes as C

import numpy as np

from . import _ffi


def auc(scores, labels, groups=None, device=0):
    """ROC AUC and per-group AUC of `scores` against the labels t = [labels > 0], ranked on the GPU, exactly (fmhip_auc_scores):
    a dict of u2, pairs, positives, negatives, groups, groups_scored, auc, gauc.  Scores are compared as float32: -0 ties with
    +0, NaN ranks below -inf and ties with NaN.  `groups`: None (one group), or one integer id in [0, 2^31) per row."""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1)
    y = np.ascontiguousarray(labels, np.float32).reshape(-1)
    if s.shape != y.shape:
        raise ValueError("scores and labels differ in length: %d, %d" % (len(s), len(y)))
    g = _ffi.group_ids(groups, len(s))
    res = _ffi.AucResult()
    _ffi.check(_ffi.load().fmhip_auc_scores(int(device), len(s), _ffi.ptr(s), _ffi.ptr(y), _ffi.ptr(g), C.byref(res)))
    return res.as_dict()


def ranking_metrics(ranks, k):
    """HitRate@k, Recall@k, Precision@k, NDCG@k, MRR and MAP of `ranks` — one integer array per context, the 0-based ranks of its
    relevant rows as ``FMModel.rankOf`` returns them — averaged over the contexts that have one (fmhip_rank_metrics; host only):
    a dict of k, contexts, skipped, relevant, hit_rate, recall, precision, ndcg, mrr, map.  A negative rank, the same rank twice
    in one context or k < 1 is refused."""
    lists = [np.asarray(r, np.int64).reshape(-1) for r in ranks]
    for r in lists:
        if len(r) and (r.min() < -2 ** 31 or r.max() >= 2 ** 31):
            raise ValueError("ranks must fit an int32")
    ptr = np.zeros(len(lists) + 1, np.int64)
    if lists:
        np.cumsum([len(r) for r in lists], out=ptr[1:])
    flat = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32)
    res = _ffi.RankMetrics()
    _ffi.check(_ffi.load().fmhip_rank_metrics(len(lists), _ffi.ptr(ptr), _ffi.ptr(flat) if len(flat) else None, int(k), C.byref(res)))
    return res.as_dict()
